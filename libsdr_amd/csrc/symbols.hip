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

// ---- a detector per channel -------------------------------------------------------------------------------------------------
// What the launch reads of channel c. origin: the handle's sample count when the channel's node was configured — its slot
// index at the call's first sample is (n_abs - origin) mod L, a closed form of two numbers the call does not upload.
struct DetChan { int kind, L, invert, lut_off; unsigned long long origin; };
struct DetPcArgs {
  const short *in; long in_stride; uint8_t *out; long out_stride;
  int N, Hs;                               // Hs = max_corr_len - 1: the history row of every channel
  unsigned long long n_abs;                // samples the handle has seen before this call
  const DetChan *ch;                       // C
  const float4 *lut;                       // the channels' LUTs, channel c's L entries from lut_off
  const short *hist_old; short *hist_new;  // C x Hs: an FSK channel uses the last L - 1 of its row
};

// fsk_detect_kernel's tile on one channel's own rows and numbers — in / out / ho / hn: the channel's rows (ho, hn: L - 1
// samples), lut: its L entries. The same statements in the same order: the order of the adds is the contract.
__device__ __forceinline__ void fsk_tile(float4 *prod, const short *in, uint8_t *out, const short *ho, short *hn, int N, int L, int phase0,
                                         const float4 *lut) {
  const int H = L - 1;
  const int i0 = blockIdx.x * SY_T;
  for (int q = threadIdx.x; q < SY_T + H; q += SY_T) {
    const int j = i0 - H + q;                                   // call-relative sample index, >= -H
    const int x = j < 0 ? (int)ho[j + H] : (j < N ? (int)in[j] : 0);
    const float4 w = lut[(unsigned)(phase0 + j + L) % (unsigned)L];
    const float xf = (float)x;
    prod[q] = make_float4(xf * w.x, xf * w.y, xf * w.z, xf * w.w);   // src/fsk.cc:70-71: one multiply per component
  }
  __syncthreads();
  const int i = i0 + (int)threadIdx.x;
  if (i < N) {
    const int p = (int)((unsigned)(phase0 + i) % (unsigned)L);
    const int base = (int)threadIdx.x + H - p;                  // LDS index of sample b = t - p (slot 0)
    float mr = 0.f, mi = 0.f, sr = 0.f, si = 0.f;
    for (int s = 0; s < L; s++) {                               // src/fsk.cc:75-79, slot order
      const float4 v = prod[base + s - (s > p ? L : 0)];
      mr += v.x; mi += v.y; sr += v.z; si += v.w;
    }
    const float f = mr * mr + mi * mi - sr * sr - si * si;      // :81-84, left to right
    out[i] = f > 0.f ? 1 : 0;
  }
  if (blockIdx.x == 0) {                                        // the history the next call reads (the other parity)
    for (int k = threadIdx.x; k < H; k += SY_T) {
      const int j = N - H + k;
      hn[k] = j >= 0 ? in[j] : ho[k + N];
    }
  }
}

// One workgroup serves one channel (blockIdx.y), so the kind and L are uniform in it: FSK and ASK rows share the launch
// without divergence inside a wave. The FSK arithmetic is fsk_tile's, the ASK row is ask_detect_kernel's expression.
__global__ __launch_bounds__(SY_T) void detectorbank_kernel(const DetPcArgs a) {
  extern __shared__ float4 prod[];   // SY_T + (the bank's largest L) - 1
  const int c = blockIdx.y;
  const DetChan ch = a.ch[c];
  const short *in = a.in + (long)c * a.in_stride;
  uint8_t *out = a.out + (long)c * a.out_stride;
  if (ch.kind == SDRHIP_DET_ASK) {
    const int i = blockIdx.x * SY_T + (int)threadIdx.x;
    if (i < a.N) out[i] = (uint8_t)((in[i] > 0 ? 1 : 0) ^ ch.invert);   // src/fsk.hh:108
    return;
  }
  const unsigned long long d = a.n_abs - ch.origin;
  const int phase0 = (d >> 32) ? (int)(d % (unsigned long long)ch.L) : (int)((unsigned)d % (unsigned)ch.L);
  const long h0 = (long)c * a.Hs + (a.Hs - (ch.L - 1));
  fsk_tile(prod, in, out, a.hist_old + h0, a.hist_new + h0, a.N, ch.L, phase0, a.lut + ch.lut_off);
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

// ---- a bit clock per channel ------------------------------------------------------------------------------------------------
struct BitChan { int L, mode; float omega0, omin, omax; };
struct FlagPcArgs {
  const uint8_t *in; long in_stride;
  int N, C, Ls;                                         // Ls = max_corr_len: the ring row of every channel
  const BitChan *ch;                                    // C
  const signed char *hist_old; signed char *hist_new;   // C x Ls: a channel uses the last L of its row
  uint4 *flags;
};

// bits_flags_kernel's tile on one channel's own rows and window — in: the channel's symbols, ho / hn: its L ring values,
// flags: its column of the mask array (stride C).
__device__ __forceinline__ void flags_tile(int *pfx, const uint8_t *in, const signed char *ho, signed char *hn, int N, int L, int C, uint4 *flags) {
  const int W = SY_T + L + 1;
  int *part = pfx + W;
  const int i0 = blockIdx.x * SY_T, j0 = i0 - L - 1;            // q = j - j0
  for (int q = threadIdx.x; q < W; q += SY_T) {
    const int j = j0 + q;
    int v = 0;
    if (j >= 0) v = j < N ? (in[j] ? 1 : -1) : 0;               // src/fsk.cc:166
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
  // (lanes beyond N vote too, on meaningless sums: the PLL kernels read only the first N - 64 g bits of a group's masks)
  const unsigned long long pos = __ballot(S > 0), tr = __ballot((Sp < 0) != (S < 0));   // :178, :190
  if ((threadIdx.x & 63) == 0 && i0 + u < N)
    flags[(long)((i0 + u) >> 6) * C] = make_uint4((unsigned)pos, (unsigned)(pos >> 32), (unsigned)tr, (unsigned)(tr >> 32));
  if (blockIdx.x == 0) {
    for (int k = threadIdx.x; k < L; k += SY_T) {
      const int j = N - L + k;
      hn[k] = j >= 0 ? (signed char)(in[j] ? 1 : -1) : ho[k + N];
    }
  }
}

__global__ __launch_bounds__(SY_T) void bitsbank_flags_kernel(const FlagPcArgs a) {
  extern __shared__ int pfx[];   // SY_T + (the bank's largest L) + 1 values, then SY_T partial sums
  const int c = blockIdx.y, L = a.ch[c].L;
  const long h0 = (long)c * a.Ls + (a.Ls - L);
  flags_tile(pfx, a.in + (long)c * a.in_stride, a.hist_old + h0, a.hist_new + h0, a.N, L, a.C, a.flags + c);
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

struct PllPcArgs {
  const uint4 *flags;
  int N, C;
  float gain;
  const BitChan *ch;                          // mode, omin and omax of the lane's channel
  float *phase, *omega; unsigned *lastbits;
  uint8_t *out; long out_stride;
  unsigned *counts;
};

// bits_pll_kernel's chain with the lane's own numbers — flags: channel c's column of the mask array (stride C). The same
// statements in the same order.
__device__ __forceinline__ void pll_lane(const uint4 *flags, int N, int C, int mode, float omin, float omax, float gain, float *phase,
                                         float *omega, unsigned *lastbits, uint8_t *row, unsigned cap, unsigned *count) {
  float ph = *phase, om = *omega;
  unsigned lb = *lastbits, o = 0;
  const double g = (double)gain;
  const int ng = (N + 63) >> 6;
  uint4 cur = flags[0];
  for (int gi = 0; gi < ng; gi++) {
    const uint4 nxt = flags[(long)min(gi + 1, ng - 1) * C];     // the next group, in flight during this one's chain
    unsigned long long pos = (unsigned long long)cur.x | ((unsigned long long)cur.y << 32);
    unsigned long long tr = (unsigned long long)cur.z | ((unsigned long long)cur.w << 32);
    const int cnt = min(64, N - 64 * gi);
    for (int k = 0; k < cnt; k++) {
      ph += om;                                                 // :171
      if (ph >= 1.f) {
        while (ph >= 1.f) ph -= 1.f;                            // :176
        lb = ((lb << 1) | (unsigned)(pos & 1ull)) & 0xffu;      // :178, a uint8_t member
        const unsigned bit = mode == SDRHIP_BITS_TRANSITION ? ((lb ^ (lb >> 1) ^ 1u) & 1u) : (lb & 1u);   // :180-186
        // cap = ceil(N * omax) + 1 is never reached: the phase enters below 1, grows by at most omax per sample and every
        // bit takes at least 1 off it, so a call emits fewer than 1 + N * omax bits. The guard only keeps a broken bound
        // from ever becoming a write past the row.
        if (o < cap) row[o++] = (uint8_t)bit;
      }
      if (tr & 1ull) {                                          // :190-198
        if ((double)ph < 0.5) om = (float)((double)om + g * (0.5 - (double)ph));
        else om = (float)((double)om - g * ((double)ph - 0.5));
        const float lo = omin < om ? om : omin;                 // std::max(_omegaMin, _omega)
        om = lo < omax ? lo : omax;                             // std::min(_omegaMax, .)
      }
      pos >>= 1; tr >>= 1;
    }
    cur = nxt;
  }
  *phase = ph; *omega = om; *lastbits = lb; *count = o;
}

// The row's capacity is the lane's own: min(ceil(N * omax[c]) + 1, out_stride), the double expression the host reports.
__global__ __launch_bounds__(64) void bitsbank_pll_kernel(const PllPcArgs a) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= a.C) return;
  const BitChan ch = a.ch[c];
  const double own = ceil((double)a.N * (double)ch.omax) + 1.0;
  const unsigned cap = own < (double)a.out_stride ? (unsigned)own : (unsigned)a.out_stride;
  pll_lane(a.flags + c, a.N, a.C, ch.mode, ch.omin, ch.omax, a.gain, a.phase + c, a.omega + c, a.lastbits + c,
           a.out + (long)c * a.out_stride, cap, a.counts + c);
}

__global__ __launch_bounds__(256) void bits_fill_kernel(float *phase, float *omega, unsigned *lastbits, float om0, int C) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c < C) { phase[c] = 0.f; omega[c] = om0; lastbits[c] = 0u; }
}

// channels c0 ... c0 + n - 1 of a per-channel handle: a fresh node's phase, rate and last bits (src/fsk.cc:127,134-136)
__global__ __launch_bounds__(256) void bitsbank_fill_kernel(float *phase, float *omega, unsigned *lastbits, const BitChan *ch, int c0, int n) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k < n) { phase[c0 + k] = 0.f; omega[c0 + k] = ch[c0 + k].omega0; lastbits[c0 + k] = 0u; }
}

constexpr int SY_MAX_L = 2048;
constexpr size_t SY_MAX_LUT_SLOTS = size_t(1) << 24;   // float4 entries of a per-channel detector's LUT buffer: 256 MiB

}  // namespace

struct sdrhip_detector {
  sdrhip_ctx *ctx = nullptr;
  int kind = 0, invert = 0, L = 1, C = 1, par = 0;
  unsigned phase = 0;   // absolute sample index mod L (every channel receives the same number of samples per call)
  size_t max_in = 0;
  DevBuf<float4> lut;
  DevBuf<short> hist[2];
  Staging stage;
  // a detector per channel (sdrhip_detectorbank_create): L is the largest corr_len of the bank's FSK channels (the
  // launch's LDS), lut holds C slots of maxL entries, hist C rows of maxL - 1 samples; kind / invert / phase are unused
  bool per_channel = false;
  int maxL = 1;
  unsigned long long n_abs = 0;   // samples per channel since create / reset
  std::vector<DetChan> chan;
  DevBuf<DetChan> chan_dev;
  void launch_per_channel(const short *in_dev, size_t N, size_t in_stride, uint8_t *out_dev, size_t out_stride) {
    DetPcArgs a;
    a.in = in_dev; a.in_stride = (long)in_stride; a.out = out_dev; a.out_stride = (long)out_stride;
    a.N = (int)N; a.Hs = maxL - 1; a.n_abs = n_abs; a.ch = chan_dev.p; a.lut = lut.p;
    a.hist_old = hist[par].p; a.hist_new = hist[par ^ 1].p;
    const size_t lds = (size_t)(SY_T + L - 1) * sizeof(float4);
    hipLaunchKernelGGL(detectorbank_kernel, dim3((unsigned)ceil_div(N, (size_t)SY_T), C), dim3(SY_T), lds, ctx->stream, a);
    SDRHIP_CHECK_HIP(hipGetLastError());
    par ^= 1;   // the state moves only for a call that was launched
    n_abs += N;
  }
  void refresh_largest() {
    L = 1;
    for (const DetChan &k : chan) if (k.kind == SDRHIP_DET_FSK) L = std::max(L, k.L);
  }
  // channel c becomes a fresh node: parameters, LUT slot, both copies of its history row, origin = now (arguments checked)
  void set_channel(int c, int kind_, const float *mark_lut, const float *space_lut, int corr_len, int invert_) {
    ctx->use();
    hipStream_t st = ctx->stream;   // stream-ordered after the launches already enqueued
    const bool fsk = kind_ == SDRHIP_DET_FSK;
    std::vector<float4> w((size_t)(fsk ? corr_len : 0));
    for (size_t i = 0; i < w.size(); i++) w[i] = make_float4(mark_lut[2 * i], mark_lut[2 * i + 1], space_lut[2 * i], space_lut[2 * i + 1]);
    const DetChan k{kind_, fsk ? corr_len : 1, !fsk && invert_ ? 1 : 0, c * maxL, n_abs};
    try {
      if (fsk) SDRHIP_CHECK_HIP(hipMemcpyAsync(lut.p + (size_t)c * maxL, w.data(), w.size() * sizeof(float4), hipMemcpyHostToDevice, st));
      if (maxL > 1)
        for (int p = 0; p < 2; p++) SDRHIP_CHECK_HIP(hipMemsetAsync(hist[p].p + (size_t)c * (maxL - 1), 0, (size_t)(maxL - 1) * sizeof(short), st));
      SDRHIP_CHECK_HIP(hipMemcpyAsync(chan_dev.p + c, &k, sizeof(DetChan), hipMemcpyHostToDevice, st));
      SDRHIP_CHECK_HIP(hipStreamSynchronize(st));
    } catch (...) {
      (void)hipStreamSynchronize(st);   // w and k are read by copies that may still be pending
      throw;
    }
    chan[c] = k;
    refresh_largest();
  }
  void launch(const short *in_dev, size_t N, size_t in_stride, uint8_t *out_dev, size_t out_stride) {
    ctx->use();
    if (N == 0) return;
    if (per_channel) return launch_per_channel(in_dev, N, in_stride, out_dev, out_stride);
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
    if (!per_channel) return;
    n_abs = 0;   // every channel a freshly configured node: its origin is the new count
    for (DetChan &k : chan) k.origin = 0;
    chan_dev.upload(chan.data(), chan.size(), ctx->stream);
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
  // a bit clock per channel (sdrhip_bitsbank_create): L and omax are the LARGEST of the bank's channels (the
  // launch's LDS, the capacity a caller's row stride needs), hist holds C rows of maxL values; mode / omega0 / omin are unused
  bool per_channel = false;
  int maxL = 1;
  double sample_rate = 0;
  std::vector<BitChan> chan;
  DevBuf<BitChan> chan_dev;
  size_t capacity(size_t n) const { return (size_t)std::ceil((double)n * (double)omax) + 1; }
  void launch_per_channel(const uint8_t *in_dev, size_t N, size_t in_stride, uint8_t *out_dev, size_t out_stride, unsigned *counts_dev) {
    FlagPcArgs f;
    f.in = in_dev; f.in_stride = (long)in_stride; f.N = (int)N; f.C = C; f.Ls = maxL; f.ch = chan_dev.p;
    f.hist_old = hist[par].p; f.hist_new = hist[par ^ 1].p; f.flags = flags.p;
    const size_t lds = (size_t)(SY_T + L + 1 + SY_T) * sizeof(int);
    hipLaunchKernelGGL(bitsbank_flags_kernel, dim3((unsigned)ceil_div(N, (size_t)SY_T), C), dim3(SY_T), lds, ctx->stream, f);
    SDRHIP_CHECK_HIP(hipGetLastError());
    PllPcArgs p;
    p.flags = flags.p; p.N = (int)N; p.C = C; p.gain = 0.0005f; p.ch = chan_dev.p;   // src/fsk.cc:132
    p.phase = phase.p; p.omega = omega.p; p.lastbits = lastbits.p;
    p.out = out_dev; p.out_stride = (long)out_stride; p.counts = counts_dev;
    hipLaunchKernelGGL(bitsbank_pll_kernel, dim3((unsigned)ceil_div((size_t)C, (size_t)64)), dim3(64), 0, ctx->stream, p);
    SDRHIP_CHECK_HIP(hipGetLastError());
    par ^= 1;   // the ring moves only for a call whose two launches went out
  }
  void refresh_largest() {
    L = 1; omax = 0.f;
    for (const BitChan &k : chan) { L = std::max(L, k.L); omax = std::max(omax, k.omax); }
  }
  void fill_per_channel(int c0, int n) {
    hipLaunchKernelGGL(bitsbank_fill_kernel, dim3((unsigned)ceil_div((size_t)n, (size_t)256)), dim3(256), 0, ctx->stream, phase.p, omega.p,
                       lastbits.p, chan_dev.p, c0, n);
    SDRHIP_CHECK_HIP(hipGetLastError());
  }
  // channel c becomes a fresh node: parameters, both copies of its ring row, phase / rate / last bits (arguments checked)
  void set_channel(int c, const BitChan &k) {
    ctx->use();
    hipStream_t st = ctx->stream;   // stream-ordered after the launches already enqueued
    try {
      for (int p = 0; p < 2; p++) SDRHIP_CHECK_HIP(hipMemsetAsync(hist[p].p + (size_t)c * maxL, 0, (size_t)maxL, st));
      SDRHIP_CHECK_HIP(hipMemcpyAsync(chan_dev.p + c, &k, sizeof(BitChan), hipMemcpyHostToDevice, st));
      fill_per_channel(c, 1);   // reads omega0 of the row just copied: behind it on the stream
      SDRHIP_CHECK_HIP(hipStreamSynchronize(st));
    } catch (...) {
      (void)hipStreamSynchronize(st);   // k is read by a copy that may still be pending
      throw;
    }
    chan[c] = k;
    refresh_largest();
  }
  void launch(const uint8_t *in_dev, size_t N, size_t in_stride, uint8_t *out_dev, size_t out_stride, unsigned *counts_dev) {
    ctx->use();
    if (N == 0) { SDRHIP_CHECK_HIP(hipMemsetAsync(counts_dev, 0, (size_t)C * sizeof(unsigned), ctx->stream)); return; }
    if (per_channel) return launch_per_channel(in_dev, N, in_stride, out_dev, out_stride, counts_dev);
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
    if (per_channel) return fill_per_channel(0, C);
    hipLaunchKernelGGL(bits_fill_kernel, dim3((unsigned)ceil_div((size_t)C, (size_t)256)), dim3(256), 0, ctx->stream, phase.p, omega.p,
                       lastbits.p, omega0, C);
    SDRHIP_CHECK_HIP(hipGetLastError());
  }
};

// what the receiver bank (rxbank.hip) asks of the handles of this file
namespace sdrhip {
sdrhip_ctx *handle_ctx(const sdrhip_detector *h) { return h->ctx; }
sdrhip_ctx *handle_ctx(const sdrhip_bits *h) { return h->ctx; }
int handle_channels(const sdrhip_detector *h) { return h->C; }
int handle_channels(const sdrhip_bits *h) { return h->C; }
size_t handle_max_in(const sdrhip_detector *h) { return h->max_in; }
size_t handle_max_in(const sdrhip_bits *h) { return h->max_in; }
}  // namespace sdrhip

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

// the argument rules of one channel's detector (create_per_channel: limit = the bank's max_corr_len, set_channel: the handle's)
static void require_detector_channel(int c, int kind, const float *mark_lut, const float *space_lut, int corr_len, int limit) {
  SDRHIP_REQUIRE(kind == SDRHIP_DET_FSK || kind == SDRHIP_DET_ASK, SDRHIP_E_INVALID, "channel %d: bad kind %d", c, kind);
  if (kind != SDRHIP_DET_FSK) return;
  SDRHIP_REQUIRE(mark_lut && space_lut, SDRHIP_E_INVALID, "channel %d: FSK needs the mark and the space LUT", c);
  SDRHIP_REQUIRE(corr_len >= 1, SDRHIP_E_INVALID, "channel %d: corr_len %d < 1", c, corr_len);
  SDRHIP_REQUIRE(corr_len <= limit, SDRHIP_E_UNSUPPORTED, "channel %d: corr_len %d > max_corr_len %d", c, corr_len, limit);
}

static void require_max_corr_len(int max_corr_len) {
  SDRHIP_REQUIRE(max_corr_len >= 0, SDRHIP_E_INVALID, "max_corr_len %d < 0", max_corr_len);
  SDRHIP_REQUIRE(max_corr_len <= SY_MAX_L, SDRHIP_E_UNSUPPORTED, "max_corr_len %d > %d", max_corr_len, SY_MAX_L);
}

int sdrhip_detectorbank_create(sdrhip_ctx *ctx, const int *kinds, const int *corr_len, const int *invert, const float *mark_luts,
                               const float *space_luts, int max_corr_len, int channels, size_t max_in, sdrhip_detector **out) {
  return guarded([&] {
    if (out) *out = nullptr;
    SDRHIP_REQUIRE(out && kinds && corr_len && invert, SDRHIP_E_INVALID, "NULL argument");
    require_channels(channels, 65535);
    require_max_in(max_in);
    require_max_corr_len(max_corr_len);
    int largest = 1;
    for (int c = 0; c < channels; c++) {
      require_detector_channel(c, kinds[c], mark_luts, space_luts, corr_len[c], max_corr_len ? max_corr_len : SY_MAX_L);
      if (kinds[c] == SDRHIP_DET_FSK) largest = std::max(largest, corr_len[c]);
    }
    // every channel owns a LUT slot of max_corr_len float4 entries: bound what one create call can allocate
    const size_t slots = (size_t)channels * (size_t)(max_corr_len ? max_corr_len : largest);
    SDRHIP_REQUIRE(slots <= SY_MAX_LUT_SLOTS, SDRHIP_E_UNSUPPORTED, "channels x max_corr_len = %zu LUT entries > %zu (256 MiB)", slots,
                   SY_MAX_LUT_SLOTS);
    require_device_for_null_ctx(ctx);
    make_handle(ctx, out, true, [&](sdrhip_detector *h) {
      h->per_channel = true; h->C = channels; h->max_in = max_in;
      h->maxL = max_corr_len ? max_corr_len : largest;
      h->chan.resize((size_t)channels);
      std::vector<float4> w((size_t)channels * h->maxL, make_float4(0.f, 0.f, 0.f, 0.f));
      size_t at = 0;   // the channel's first (re, im) pair in the concatenated LUTs
      for (int c = 0; c < channels; c++) {
        const bool fsk = kinds[c] == SDRHIP_DET_FSK;
        h->chan[c] = DetChan{kinds[c], fsk ? corr_len[c] : 1, !fsk && invert[c] ? 1 : 0, c * h->maxL, 0ull};
        if (!fsk) continue;
        for (int i = 0; i < corr_len[c]; i++, at++)
          w[(size_t)c * h->maxL + i] = make_float4(mark_luts[2 * at], mark_luts[2 * at + 1], space_luts[2 * at], space_luts[2 * at + 1]);
      }
      h->refresh_largest();
      h->lut.alloc(w.size());
      h->lut.upload(w.data(), w.size(), ctx->stream);
      h->chan_dev.alloc((size_t)channels);
      for (int p = 0; p < 2; p++) h->hist[p].alloc((size_t)channels * (size_t)std::max(h->maxL - 1, 1));
      h->reset();
    });
  });
}

int sdrhip_detectorbank_set_channel(sdrhip_detector *h, int channel, int kind, const float *mark_lut, const float *space_lut, int corr_len,
                                    int invert) {
  return guarded([&] {
    SDRHIP_REQUIRE(h, SDRHIP_E_INVALID, "handle is NULL");
    SDRHIP_REQUIRE(h->per_channel, SDRHIP_E_UNSUPPORTED,
                   "the handle has one detector for all channels (sdrhip_detectorbank_create makes one per channel)");
    require_channel_range(h, channel);
    require_detector_channel(channel, kind, mark_lut, space_lut, corr_len, h->maxL);
    h->set_channel(channel, kind, mark_lut, space_lut, corr_len, invert);
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
    write_names(h, buf, len, [&] {
      return h->per_channel ? "detectorbank_kernel" : h->kind == SDRHIP_DET_ASK ? "ask_detect_kernel" : "fsk_detect_kernel";
    });
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

// BitStream::config's numbers for one (sample rate, baud rate, mode), with their argument rules; limit: the longest window
static BitChan bit_clock(double sample_rate, float baud, int mode, int limit) {
  SDRHIP_REQUIRE(mode == SDRHIP_BITS_NORMAL || mode == SDRHIP_BITS_TRANSITION, SDRHIP_E_INVALID, "bad mode %d", mode);
  SDRHIP_REQUIRE(sample_rate > 0 && baud > 0, SDRHIP_E_INVALID, "sample rate and baud rate must be positive");
  const double l = sample_rate / baud;
  SDRHIP_REQUIRE(l >= 1.0, SDRHIP_E_INVALID, "fewer than one symbol per bit");
  SDRHIP_REQUIRE(l < limit + 1, SDRHIP_E_UNSUPPORTED, "more than %d symbols per bit", limit);
  BitChan k;
  k.L = int(l);                                                  // src/fsk.cc:122
  k.mode = mode;
  k.omega0 = (float)(baud / sample_rate);                        // :127, float = float / double
  k.omin = (float)((double)k.omega0 - 0.005 * (double)k.omega0); // :129
  k.omax = (float)((double)k.omega0 + 0.005 * (double)k.omega0); // :130
  return k;
}

int sdrhip_bits_create(sdrhip_ctx *ctx, double sample_rate, float baud, int mode, int channels, size_t max_in, sdrhip_bits **out) {
  return guarded([&] {
    make_handle(ctx, out, true, [&](sdrhip_bits *h) {
      SDRHIP_REQUIRE(mode == SDRHIP_BITS_NORMAL || mode == SDRHIP_BITS_TRANSITION, SDRHIP_E_INVALID, "bad mode %d", mode);
      SDRHIP_REQUIRE(sample_rate > 0 && baud > 0, SDRHIP_E_INVALID, "sample rate and baud rate must be positive");
      require_channels(channels, 65535);
      require_max_in(max_in);
      const BitChan k = bit_clock(sample_rate, baud, mode, SY_MAX_L);
      h->mode = mode; h->C = channels; h->max_in = max_in;
      h->L = k.L; h->omega0 = k.omega0; h->omin = k.omin; h->omax = k.omax;
      for (int p = 0; p < 2; p++) h->hist[p].alloc((size_t)channels * (size_t)h->L);
      h->flags.alloc((size_t)channels * ceil_div(max_in, (size_t)64));
      h->phase.alloc(channels); h->omega.alloc(channels); h->lastbits.alloc(channels); h->counts.alloc(channels);
      h->reset();
    });
  });
}

int sdrhip_bitsbank_create(sdrhip_ctx *ctx, double sample_rate, const float *baud, const int *mode, int channels, size_t max_in,
                           int max_corr_len, sdrhip_bits **out) {
  return guarded([&] {
    if (out) *out = nullptr;
    SDRHIP_REQUIRE(out && baud && mode, SDRHIP_E_INVALID, "NULL argument");
    require_channels(channels, 65535);
    require_max_in(max_in);
    require_max_corr_len(max_corr_len);
    std::vector<BitChan> chan((size_t)channels);
    int largest = 1;
    for (int c = 0; c < channels; c++) {
      chan[c] = bit_clock(sample_rate, baud[c], mode[c], max_corr_len ? max_corr_len : SY_MAX_L);
      largest = std::max(largest, chan[c].L);
    }
    require_device_for_null_ctx(ctx);
    make_handle(ctx, out, true, [&](sdrhip_bits *h) {
      h->per_channel = true; h->C = channels; h->max_in = max_in; h->sample_rate = sample_rate;
      h->maxL = max_corr_len ? max_corr_len : largest;
      h->chan = chan;
      h->refresh_largest();
      h->chan_dev.alloc((size_t)channels);
      h->chan_dev.upload(h->chan.data(), h->chan.size(), ctx->stream);
      for (int p = 0; p < 2; p++) h->hist[p].alloc((size_t)channels * (size_t)h->maxL);
      h->flags.alloc((size_t)channels * ceil_div(max_in, (size_t)64));
      h->phase.alloc(channels); h->omega.alloc(channels); h->lastbits.alloc(channels); h->counts.alloc(channels);
      h->reset();
    });
  });
}

static void require_per_channel_bits(const sdrhip_bits *h, int channel) {
  SDRHIP_REQUIRE(h, SDRHIP_E_INVALID, "handle is NULL");
  SDRHIP_REQUIRE(h->per_channel, SDRHIP_E_UNSUPPORTED,
                 "the handle has one bit clock for all channels (sdrhip_bitsbank_create makes one per channel)");
  require_channel_range(h, channel);
}

int sdrhip_bitsbank_set_channel(sdrhip_bits *h, int channel, float baud, int mode) {
  return guarded([&] {
    require_per_channel_bits(h, channel);
    h->set_channel(channel, bit_clock(h->sample_rate, baud, mode, h->maxL));
  });
}

int sdrhip_bitsbank_channel_info(sdrhip_bits *h, int channel, size_t n_in, int *corr_len, float *omega_min, float *omega_max, size_t *cap) {
  return guarded([&] {
    require_per_channel_bits(h, channel);
    const BitChan &k = h->chan[channel];
    if (corr_len) *corr_len = k.L;
    if (omega_min) *omega_min = k.omin;
    if (omega_max) *omega_max = k.omax;
    if (cap) *cap = (size_t)std::ceil((double)n_in * (double)k.omax) + 1;
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
    // (a set_channel to a faster baud rate raises capacity(max_in): the one case in which the staged rows grow)
    process_counted(h, sym_host, n, in_stride, 1, bits_host, out_stride, counts_host, [&](void *in, uint8_t *out, size_t cap) {
      h->launch(static_cast<const uint8_t *>(in), n, n, out, cap, h->counts.p);
    });
  });
}

int sdrhip_bits_kernel_names(sdrhip_bits *h, char *buf, size_t len) {
  return guarded([&] {
    write_names(h, buf, len, [&] { return h->per_channel ? "bitsbank_pll_kernel,bitsbank_flags_kernel" : "bits_pll_kernel,bits_flags_kernel"; });
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
