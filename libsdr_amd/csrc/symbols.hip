// symbols.hip — audio to bits on the device: FSKDetector, ASKDetector and BitStream.
//
// Replaces (reference, file:line):
//   FSKDetector::_process / process        src/fsk.cc:68-95
//   ASKDetector<int16_t>::process          src/fsk.hh:106-111
//   BitStream::process                     src/fsk.cc:157-202
//
// FSKDetector is a sliding correlation whose float sum runs over the node's ring in SLOT order, not in time order
// (src/fsk.cc:75-79), and whose sign test has no tolerance (:81-86): the order of the adds is the contract. On the absolute
// sample index t (counted from the last reset), with L = corrLen, p = t mod L and b = t - p, slot i holds the product
// P[t'] = float(x[t']) * LUT[t' mod L] of the newest t' <= t congruent to i — so output t is
//   ((0 + P[b] + ... + P[t]) + P[t-L+1] + ... + P[b-1]),
// which needs only the L - 1 samples before t: tiles of a row are independent given an L - 1 sample halo. Slots never
// written hold +0, as a zero sample does (a product of -0 changes no sum that started at +0).
// The file is compiled with -ffp-contract=off (csrc/Makefile): the products and the adds stay separate operations, as in
// the reference's build (no -march, no FMA), and gfx950 code keeps float denormals by default.
//
// BitStream keeps a window sum of +/-1 symbols (exact, order-free) and a float/double PLL recursion (sequential). Two
// launches: bits_flags_kernel computes, across lanes, for every sample whether the window sum is positive and whether its
// sign changed, 2 bits per sample gathered with wave ballots; bits_pll_kernel walks one channel per lane over those masks.
#include <cmath>

#include "sdrhip_internal.hpp"
#include "entry.hpp"

using namespace sdrhip;

namespace {

constexpr int SY_T = 256;   // outputs per workgroup (one thread each)

struct DetArgs {
  const short *in; long in_stride; uint8_t *out; long out_stride;
  int N, L, phase0, invert;
  const float4 *lut;                       // L x (mark.re, mark.im, space.re, space.im)
  const short *hist_old; short *hist_new;  // C x (L - 1): the samples before the call / after it
};

// One workgroup: SY_T consecutive outputs of one channel. The SY_T + L - 1 products are staged once in LDS (one float4 per
// sample: both tones), then every lane adds its L slots in the reference's order.
__global__ __launch_bounds__(SY_T) void fsk_detect_kernel(const DetArgs a) {
  extern __shared__ float4 prod[];   // SY_T + L - 1
  const int c = blockIdx.y, L = a.L, H = L - 1;
  const short *in = a.in + (long)c * a.in_stride;
  const short *ho = a.hist_old + (long)c * H;
  const int i0 = blockIdx.x * SY_T;
  for (int q = threadIdx.x; q < SY_T + H; q += SY_T) {
    const int j = i0 - H + q;                                   // call-relative sample index, >= -H
    const int x = j < 0 ? (int)ho[j + H] : (j < a.N ? (int)in[j] : 0);
    const float4 w = a.lut[(unsigned)(a.phase0 + j + L) % (unsigned)L];
    const float xf = (float)x;
    prod[q] = make_float4(xf * w.x, xf * w.y, xf * w.z, xf * w.w);   // src/fsk.cc:70-71: one multiply per component
  }
  __syncthreads();
  const int i = i0 + (int)threadIdx.x;
  if (i < a.N) {
    const int p = (int)((unsigned)(a.phase0 + i) % (unsigned)L);
    const int base = (int)threadIdx.x + H - p;                  // LDS index of sample b = t - p (slot 0)
    float mr = 0.f, mi = 0.f, sr = 0.f, si = 0.f;
    for (int s = 0; s < L; s++) {                               // src/fsk.cc:75-79, slot order
      const float4 v = prod[base + s - (s > p ? L : 0)];
      mr += v.x; mi += v.y; sr += v.z; si += v.w;
    }
    const float f = mr * mr + mi * mi - sr * sr - si * si;      // :81-84, left to right
    a.out[(long)c * a.out_stride + i] = f > 0.f ? 1 : 0;
  }
  if (blockIdx.x == 0) {                                        // the history the next call reads (the other parity)
    short *hn = a.hist_new + (long)c * H;
    for (int k = threadIdx.x; k < H; k += SY_T) {
      const int j = a.N - H + k;
      hn[k] = j >= 0 ? in[j] : ho[k + a.N];
    }
  }
}

// ASKDetector<int16_t>: (x > 0) ^ invert (src/fsk.hh:108)
__global__ __launch_bounds__(SY_T) void ask_detect_kernel(const DetArgs a) {
  const int c = blockIdx.y;
  const short *in = a.in + (long)c * a.in_stride;
  uint8_t *out = a.out + (long)c * a.out_stride;
  for (int i = blockIdx.x * SY_T + threadIdx.x; i < a.N; i += gridDim.x * SY_T) out[i] = (uint8_t)((in[i] > 0 ? 1 : 0) ^ a.invert);
}

struct FlagArgs {
  const uint8_t *in; long in_stride;
  int N, L, C;
  const signed char *hist_old; signed char *hist_new;   // C x L: the last L ring values (+1, -1, 0 before the ring fills)
  uint4 *flags;                                         // [group of 64 samples][channel]: (positive mask, sign-change mask)
};

// Window sums by differences of a prefix sum over the tile's SY_T + L + 1 ring values (integers: exact whatever the order).
// S(i) = sum of the L values ending at sample i is _symSum after the ring update of sample i, S(i - 1) is _lastSymSum
// (src/fsk.cc:164-168); before the call's first sample S(-1) is the sum of the carried ring.
__global__ __launch_bounds__(SY_T) void bits_flags_kernel(const FlagArgs a) {
  extern __shared__ int pfx[];   // SY_T + L + 1 values, then SY_T partial sums
  const int c = blockIdx.y, L = a.L, W = SY_T + L + 1;
  int *part = pfx + W;
  const uint8_t *in = a.in + (long)c * a.in_stride;
  const signed char *ho = a.hist_old + (long)c * L;
  const int i0 = blockIdx.x * SY_T, j0 = i0 - L - 1;            // q = j - j0
  for (int q = threadIdx.x; q < W; q += SY_T) {
    const int j = j0 + q;
    int v = 0;
    if (j >= 0) v = j < a.N ? (in[j] ? 1 : -1) : 0;             // src/fsk.cc:166
    else if (j >= -L) v = (int)ho[j + L];
    pfx[q] = v;
  }
  __syncthreads();
  const int m = (W + SY_T - 1) / SY_T, q0 = min((int)threadIdx.x * m, W), q1 = min(q0 + m, W);
  int s = 0;
  for (int q = q0; q < q1; q++) s += pfx[q];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int off = 1; off < SY_T; off <<= 1) {
    const int add = (int)threadIdx.x >= off ? part[threadIdx.x - off] : 0;
    __syncthreads();
    part[threadIdx.x] += add;
    __syncthreads();
  }
  int run = threadIdx.x ? part[threadIdx.x - 1] : 0;
  for (int q = q0; q < q1; q++) { run += pfx[q]; pfx[q] = run; }
  __syncthreads();
  const int u = threadIdx.x;                                    // sample i0 + u sits at q = u + L + 1
  const int S = pfx[u + L + 1] - pfx[u + 1], Sp = pfx[u + L] - pfx[u];
  // (lanes beyond N vote too, on meaningless sums: bits_pll_kernel reads only the first N - 64 g bits of a group's masks)
  const unsigned long long pos = __ballot(S > 0), tr = __ballot((Sp < 0) != (S < 0));   // :178, :190
  if ((threadIdx.x & 63) == 0 && i0 + u < a.N)
    a.flags[(long)((i0 + u) >> 6) * a.C + c] = make_uint4((unsigned)pos, (unsigned)(pos >> 32), (unsigned)tr, (unsigned)(tr >> 32));
  if (blockIdx.x == 0) {
    signed char *hn = a.hist_new + (long)c * L;
    for (int k = threadIdx.x; k < L; k += SY_T) {
      const int j = a.N - L + k;
      hn[k] = j >= 0 ? (signed char)(in[j] ? 1 : -1) : ho[k + a.N];
    }
  }
}

struct PllArgs {
  const uint4 *flags;
  int N, C, mode;
  float omin, omax, gain;
  float *phase, *omega; unsigned *lastbits;   // per channel, updated in place (one lane per channel)
  uint8_t *out; long out_stride; unsigned cap;
  unsigned *counts;
};

// The PLL as a latency chain, one lane per channel (as deemph_i16_seq_kernel): _phase and _omega are floats, the
// correction is evaluated in double and narrowed (src/fsk.cc:171-198, _pllGain a float member, 0.5 a double constant).
__global__ __launch_bounds__(64) void bits_pll_kernel(const PllArgs a) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= a.C) return;
  float ph = a.phase[c], om = a.omega[c];
  unsigned lb = a.lastbits[c], o = 0;
  const double g = (double)a.gain;
  uint8_t *row = a.out + (long)c * a.out_stride;
  const int ng = (a.N + 63) >> 6;
  uint4 cur = a.flags[c];
  for (int gi = 0; gi < ng; gi++) {
    const uint4 nxt = a.flags[(long)min(gi + 1, ng - 1) * a.C + c];   // the next group, in flight during this one's chain
    unsigned long long pos = (unsigned long long)cur.x | ((unsigned long long)cur.y << 32);
    unsigned long long tr = (unsigned long long)cur.z | ((unsigned long long)cur.w << 32);
    const int cnt = min(64, a.N - 64 * gi);
    for (int k = 0; k < cnt; k++) {
      ph += om;                                                 // :171
      if (ph >= 1.f) {
        while (ph >= 1.f) ph -= 1.f;                            // :176
        lb = ((lb << 1) | (unsigned)(pos & 1ull)) & 0xffu;      // :178, a uint8_t member
        const unsigned bit = a.mode == SDRHIP_BITS_TRANSITION ? ((lb ^ (lb >> 1) ^ 1u) & 1u) : (lb & 1u);   // :180-186
        // cap = ceil(N * omax) + 1 is never reached: the phase enters below 1, grows by at most omax per sample and every
        // bit takes at least 1 off it, so a call emits fewer than 1 + N * omax bits. The guard only keeps a broken bound
        // from ever becoming a write past the row.
        if (o < a.cap) row[o++] = (uint8_t)bit;
      }
      if (tr & 1ull) {                                          // :190-198
        if ((double)ph < 0.5) om = (float)((double)om + g * (0.5 - (double)ph));
        else om = (float)((double)om - g * ((double)ph - 0.5));
        const float lo = a.omin < om ? om : a.omin;             // std::max(_omegaMin, _omega)
        om = lo < a.omax ? lo : a.omax;                         // std::min(_omegaMax, .)
      }
      pos >>= 1; tr >>= 1;
    }
    cur = nxt;
  }
  a.phase[c] = ph; a.omega[c] = om; a.lastbits[c] = lb; a.counts[c] = o;
}

__global__ __launch_bounds__(256) void bits_fill_kernel(float *phase, float *omega, unsigned *lastbits, float om0, int C) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c < C) { phase[c] = 0.f; omega[c] = om0; lastbits[c] = 0u; }
}

constexpr int SY_MAX_L = 2048;

}  // namespace

struct sdrhip_detector {
  sdrhip_ctx *ctx = nullptr;
  int kind = 0, invert = 0, L = 1, C = 1, par = 0;
  unsigned phase = 0;   // absolute sample index mod L (every channel receives the same number of samples per call)
  size_t max_in = 0;
  DevBuf<float4> lut;
  DevBuf<short> hist[2];
  Staging stage;
  void launch(const short *in_dev, size_t N, size_t in_stride, uint8_t *out_dev, size_t out_stride) {
    ctx->use();
    if (N == 0) return;
    DetArgs a;
    a.in = in_dev; a.in_stride = (long)in_stride; a.out = out_dev; a.out_stride = (long)out_stride;
    a.N = (int)N; a.L = L; a.phase0 = (int)phase; a.invert = invert;
    a.lut = lut.p; a.hist_old = hist[par].p; a.hist_new = hist[par ^ 1].p;
    if (kind == SDRHIP_DET_ASK) {
      const unsigned bx = (unsigned)std::min<size_t>(ceil_div(N, (size_t)SY_T), 64);
      hipLaunchKernelGGL(ask_detect_kernel, dim3(bx, C), dim3(SY_T), 0, ctx->stream, a);
    } else {
      const size_t lds = (size_t)(SY_T + L - 1) * sizeof(float4);
      hipLaunchKernelGGL(fsk_detect_kernel, dim3((unsigned)ceil_div(N, (size_t)SY_T), C), dim3(SY_T), lds, ctx->stream, a);
    }
    SDRHIP_CHECK_HIP(hipGetLastError());
    if (kind == SDRHIP_DET_FSK) {   // the state moves only for a call that was launched
      par ^= 1;
      phase = (unsigned)((phase + N) % (size_t)L);
    }
  }
  void reset() {
    ctx->use();
    for (int p = 0; p < 2; p++) hist[p].zero(ctx->stream);
    phase = 0;
  }
};

struct sdrhip_bits {
  sdrhip_ctx *ctx = nullptr;
  int mode = 0, L = 1, C = 1, par = 0;
  float omega0 = 0.f, omin = 0.f, omax = 0.f;
  size_t max_in = 0;
  DevBuf<signed char> hist[2];
  DevBuf<uint4> flags;
  DevBuf<float> phase, omega;
  DevBuf<unsigned> lastbits, counts;
  Staging stage;
  size_t capacity(size_t n) const { return (size_t)std::ceil((double)n * (double)omax) + 1; }
  void launch(const uint8_t *in_dev, size_t N, size_t in_stride, uint8_t *out_dev, size_t out_stride, unsigned *counts_dev) {
    ctx->use();
    if (N == 0) { SDRHIP_CHECK_HIP(hipMemsetAsync(counts_dev, 0, (size_t)C * sizeof(unsigned), ctx->stream)); return; }
    FlagArgs f;
    f.in = in_dev; f.in_stride = (long)in_stride; f.N = (int)N; f.L = L; f.C = C;
    f.hist_old = hist[par].p; f.hist_new = hist[par ^ 1].p; f.flags = flags.p;
    const size_t lds = (size_t)(SY_T + L + 1 + SY_T) * sizeof(int);
    hipLaunchKernelGGL(bits_flags_kernel, dim3((unsigned)ceil_div(N, (size_t)SY_T), C), dim3(SY_T), lds, ctx->stream, f);
    SDRHIP_CHECK_HIP(hipGetLastError());
    PllArgs p;
    p.flags = flags.p; p.N = (int)N; p.C = C; p.mode = mode; p.omin = omin; p.omax = omax; p.gain = 0.0005f;   // src/fsk.cc:132
    p.phase = phase.p; p.omega = omega.p; p.lastbits = lastbits.p;
    p.out = out_dev; p.out_stride = (long)out_stride; p.cap = (unsigned)std::min<size_t>(capacity(N), out_stride);
    p.counts = counts_dev;
    hipLaunchKernelGGL(bits_pll_kernel, dim3((unsigned)ceil_div((size_t)C, (size_t)64)), dim3(64), 0, ctx->stream, p);
    SDRHIP_CHECK_HIP(hipGetLastError());
    par ^= 1;   // the ring moves only for a call whose two launches went out
  }
  void reset() {
    ctx->use();
    for (int p = 0; p < 2; p++) hist[p].zero(ctx->stream);
    hipLaunchKernelGGL(bits_fill_kernel, dim3((unsigned)ceil_div((size_t)C, (size_t)256)), dim3(256), 0, ctx->stream, phase.p, omega.p,
                       lastbits.p, omega0, C);
    SDRHIP_CHECK_HIP(hipGetLastError());
  }
};

extern "C" {

int sdrhip_detector_create(sdrhip_ctx *ctx, int kind, const float *mark_lut, const float *space_lut, int corr_len, int invert,
                           int channels, size_t max_in, sdrhip_detector **out) {
  return guarded([&] {
    make_handle(ctx, out, true, [&](sdrhip_detector *h) {
      SDRHIP_REQUIRE(kind == SDRHIP_DET_FSK || kind == SDRHIP_DET_ASK, SDRHIP_E_INVALID, "bad kind %d", kind);
      require_channels(channels, 65535);
      require_max_in(max_in);
      h->kind = kind; h->invert = invert ? 1 : 0; h->C = channels; h->max_in = max_in;
      if (kind != SDRHIP_DET_FSK) return;
      SDRHIP_REQUIRE(mark_lut && space_lut, SDRHIP_E_INVALID, "FSK needs the mark and the space LUT");
      SDRHIP_REQUIRE(corr_len >= 1, SDRHIP_E_INVALID, "corr_len %d < 1", corr_len);
      SDRHIP_REQUIRE(corr_len <= SY_MAX_L, SDRHIP_E_UNSUPPORTED, "corr_len %d > %d", corr_len, SY_MAX_L);
      h->L = corr_len;
      std::vector<float4> w((size_t)corr_len);
      for (int i = 0; i < corr_len; i++) w[i] = make_float4(mark_lut[2 * i], mark_lut[2 * i + 1], space_lut[2 * i], space_lut[2 * i + 1]);
      h->lut.alloc((size_t)corr_len);
      h->lut.upload(w.data(), (size_t)corr_len, ctx->stream);
      for (int p = 0; p < 2; p++) h->hist[p].alloc((size_t)channels * (size_t)std::max(corr_len - 1, 1));
      h->reset();
    });
  });
}

int sdrhip_detector_process_dev(sdrhip_detector *h, const int16_t *in_dev, size_t n, size_t in_stride, uint8_t *out_dev,
                                size_t out_stride) {
  return guarded([&] {
    Range roctx_range("sdrhip_detector_process_dev");
    if (!call_begin(h, "n", n, in_dev, out_dev)) return;
    const Strides s = call_strides("n", n, in_stride, n, out_stride, STRIDES_TOGETHER);
    require_disjoint(in_dev, s.in, n, 2, out_dev, s.out, n, 1, (size_t)h->C);
    h->launch(in_dev, n, s.in, out_dev, s.out);
  });
}

int sdrhip_detector_process(sdrhip_detector *h, const int16_t *in_host, size_t n, size_t in_stride, uint8_t *out_host,
                            size_t out_stride) {
  return guarded([&] {
    Range roctx_range("sdrhip_detector_process");
    if (!call_begin(h, "n", n, in_host, out_host)) return;
    const Strides s = call_strides("n", n, in_stride, n, out_stride, STRIDES_TOGETHER);
    const size_t C = (size_t)h->C;
    run_staged(h->ctx, h->stage, C * h->max_in * 2, C * h->max_in, {in_host, s.in * 2, n * 2, C}, {out_host, s.out, n, C},
               [&](void *in, void *out) {
                 h->launch(static_cast<const short *>(in), n, n, static_cast<uint8_t *>(out), n);
                 return n;
               });
  });
}

int sdrhip_detector_kernel_names(sdrhip_detector *h, char *buf, size_t len) {
  return guarded([&] {
    SDRHIP_REQUIRE(h && buf && len, SDRHIP_E_INVALID, "NULL argument");
    snprintf(buf, len, "%s", h->kind == SDRHIP_DET_ASK ? "ask_detect_kernel" : "fsk_detect_kernel");
  });
}

int sdrhip_detector_reset(sdrhip_detector *h) {
  return guarded([&] {
    use_handle(h);
    h->reset();
  });
}

int sdrhip_detector_destroy(sdrhip_detector *h) {
  return guarded([&] { destroy_handle(h); });
}

int sdrhip_bits_create(sdrhip_ctx *ctx, double sample_rate, float baud, int mode, int channels, size_t max_in, sdrhip_bits **out) {
  return guarded([&] {
    make_handle(ctx, out, true, [&](sdrhip_bits *h) {
      SDRHIP_REQUIRE(mode == SDRHIP_BITS_NORMAL || mode == SDRHIP_BITS_TRANSITION, SDRHIP_E_INVALID, "bad mode %d", mode);
      SDRHIP_REQUIRE(sample_rate > 0 && baud > 0, SDRHIP_E_INVALID, "sample rate and baud rate must be positive");
      require_channels(channels, 65535);
      require_max_in(max_in);
      const double l = sample_rate / baud;
      SDRHIP_REQUIRE(l >= 1.0, SDRHIP_E_INVALID, "fewer than one symbol per bit");
      SDRHIP_REQUIRE(l < SY_MAX_L + 1, SDRHIP_E_UNSUPPORTED, "more than %d symbols per bit", SY_MAX_L);
      h->mode = mode; h->C = channels; h->max_in = max_in;
      h->L = int(l);                                                       // src/fsk.cc:122
      h->omega0 = (float)(baud / sample_rate);                             // :127, float = float / double
      h->omin = (float)((double)h->omega0 - 0.005 * (double)h->omega0);    // :129
      h->omax = (float)((double)h->omega0 + 0.005 * (double)h->omega0);    // :130
      for (int p = 0; p < 2; p++) h->hist[p].alloc((size_t)channels * (size_t)h->L);
      h->flags.alloc((size_t)channels * ceil_div(max_in, (size_t)64));
      h->phase.alloc(channels); h->omega.alloc(channels); h->lastbits.alloc(channels); h->counts.alloc(channels);
      h->reset();
    });
  });
}

int sdrhip_bits_corr_len(sdrhip_bits *h, int *corr_len) {
  return guarded([&] {
    SDRHIP_REQUIRE(h && corr_len, SDRHIP_E_INVALID, "NULL argument");
    *corr_len = h->L;
  });
}

int sdrhip_bits_out_capacity(sdrhip_bits *h, size_t n_in, size_t *cap) {
  return guarded([&] {
    SDRHIP_REQUIRE(h && cap, SDRHIP_E_INVALID, "NULL argument");
    *cap = h->capacity(n_in);
  });
}

// (BitStream's head is its own: the counts pointer is checked with the handle, and an empty call still zeroes the counts)
int sdrhip_bits_process_dev(sdrhip_bits *h, const uint8_t *sym_dev, size_t n, size_t in_stride, uint8_t *bits_dev, size_t out_stride,
                            uint32_t *counts_dev) {
  return guarded([&] {
    Range roctx_range("sdrhip_bits_process_dev");
    SDRHIP_REQUIRE(h && counts_dev, SDRHIP_E_INVALID, "NULL argument");
    Strides s{in_stride, out_stride};
    if (call_begin(h, "n", n, sym_dev, bits_dev)) {
      s = call_strides("n", n, in_stride, h->capacity(n), out_stride, STRIDE_IN | STRIDE_OUT, "capacity");
      require_disjoint(sym_dev, s.in, n, 1, bits_dev, s.out, h->capacity(n), 1, (size_t)h->C);
    }
    h->launch(sym_dev, n, s.in, bits_dev, s.out, counts_dev);
  });
}

int sdrhip_bits_process(sdrhip_bits *h, const uint8_t *sym_host, size_t n, size_t in_stride, uint8_t *bits_host, size_t out_stride,
                        uint32_t *counts_host) {
  return guarded([&] {
    Range roctx_range("sdrhip_bits_process");
    SDRHIP_REQUIRE(h && counts_host, SDRHIP_E_INVALID, "NULL argument");
    if (!call_begin(h, "n", n, sym_host, bits_host)) { memset(counts_host, 0, (size_t)h->C * sizeof(uint32_t)); return; }
    const size_t cap = h->capacity(n), C = (size_t)h->C;
    const Strides s = call_strides("n", n, in_stride, cap, out_stride, STRIDE_IN | STRIDE_OUT, "capacity");
    run_staged(h->ctx, h->stage, C * h->max_in, C * h->capacity(h->max_in), {sym_host, s.in, n, C}, {bits_host, s.out, cap, C},
               [&](void *in, void *out) {
                 h->stage.out.zero(h->ctx->stream);   // the bytes of a row behind counts[c] reach the caller as zeros
                 h->launch(static_cast<const uint8_t *>(in), n, n, static_cast<uint8_t *>(out), cap, h->counts.p);
                 SDRHIP_CHECK_HIP(hipMemcpyAsync(counts_host, h->counts.p, C * sizeof(uint32_t), hipMemcpyDeviceToHost, h->ctx->stream));
                 return cap;
               });
  });
}

int sdrhip_bits_kernel_names(sdrhip_bits *h, char *buf, size_t len) {
  return guarded([&] {
    SDRHIP_REQUIRE(h && buf && len, SDRHIP_E_INVALID, "NULL argument");
    snprintf(buf, len, "bits_pll_kernel,bits_flags_kernel");
  });
}

int sdrhip_bits_reset(sdrhip_bits *h) {
  return guarded([&] {
    use_handle(h);
    h->reset();
  });
}

int sdrhip_bits_destroy(sdrhip_bits *h) {
  return guarded([&] { destroy_handle(h); });
}

}  // extern "C"
