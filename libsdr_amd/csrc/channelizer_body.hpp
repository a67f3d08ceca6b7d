// channelizer_body.hpp — the polyphase channelizer's kernel body, shared by channelizer.hip (complex float rows out),
// chanaudio.hip (demodulated int16 rows out) and chanpower.hip (no rows out: per-channel sums of |y|^2). One form serves every
// M: a workgroup of CH_THREADS lanes takes a tile of T consecutive output times (and, where the epilogue asks for it, `halo`
// output times before them),
//   1  all lanes: element (tt, r) of the tile, r fastest — the branch sum u[r] = sum_p h[p M + r] x[t - p M - r] as a float fma
//      chain over global reads (taps and input are contiguous in r; the row is re-read P times per output time, from L1 / L2) —
//      written into image tt at the digit-reversed position of (r - t) mod M: the circular shift by the absolute time costs
//      an index, and inverse_dit's input order another;
//   2  all lanes: the backward decimation-in-time passes of fftgen.hpp over the images at once — its butterflies (dft_small,
//      gmulc) and its plan's roots, a pass's lane loop running over (image, butterfly) so that a workgroup is busy on an 8-point
//      transform as well;
//   3  the epilogue policy: what becomes of the spectra in LDS (image tt is at img + tt * ld, natural order), and what of the
//      handle's state is rolled. A policy E has
//        int  halo(const ChArgs &, int j0)                           images wanted before output time j0 (0 or 1, uniform)
//        void store(const ChArgs &, const float2 *img, int j0, int Tc, int halo, int tid)   the tile's outputs; image halo + tt
//                                                                    holds output time j0 + tt
//        void roll<I>(const ChArgs &, int tid)                       every block, behind its tiles (ch_roll_tail at least)
// The three phases are ONE function, ch_tile. ch_body gives a workgroup one tile; ch_body_walk(W) walks the first W workgroups of
// a launch over the tiles with stride W — chanpower.hip's launch of fewer workgroups than tiles (W = gridDim.x), and a member's
// row of a group launch (sdrhip_changroup.h: ChGroupArgs, and at the end of this file the group's host layer).
// An output time is computed with the same operations in the same order whichever policy asks and wherever it lies in a tile
// (the library is built with -ffp-contract=off, and the one fused operation is written as such), so the kernel families
// agree bit for bit on the spectra.
// The input is read at [0, n) and the tail at [0, n_taps - 1) only: the first output time of a call is not before its first
// sample, the last not behind its last, and terms at l >= n_taps are skipped.
//
// The real-input form (sdrhip_chanreal.h; I = short or float, ChIn<I>::real) is the same function, apart at three `if constexpr`:
// a real branch sum (one fma per term, a float tail) packed as component jw & 1 of element jw >> 1 of an M / 2-point image; behind
// the M / 2-point plan's passes the untangling pass ch_untangle, which leaves the M / 2 + 1 distinct channels at img[tt ld + k],
// natural order — what the epilogue policies read; and a policy is handed the arguments with M replaced by the channels an image
// holds, M / 2 + 1 (ch_epi_args), so its per-channel loops and strides need no second form. ChArgs is one struct for both.
#pragma once
#include "sdrhip_internal.hpp"
#include "sdrhip_channelizer.h"
#include "sdrhip_changroup.h"
#include "entry.hpp"
#include "fftgen.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace sdrhip {

constexpr int CH_THREADS = fftgen::GT, CH_TMAX = 256;
constexpr int CH_M_MIN = 2, CH_M_MIN_REAL = 4, CH_M_MAX = 4096, CH_BRANCH_MAX = 64;
constexpr int CH_ELEMS_SMALL = 4096, CH_ELEMS_LARGE = 8192, CH_M_SMALL = 512;   // complex elements of LDS a workgroup's T images take

struct ChArgs {
  fftgen::GenDev<float2> fft;
  const void *in;          // [n] of the input type
  const float2 *hist;      // [HH] the tail before the call, oldest first
  float2 *hist_new;        // [HH] the tail behind it
  const float *taps;       // [n_taps]
  const int *invperm;      // [M] natural index -> position in inverse_dit's input (a real row: [M / 2], and behind them, at
                           // the next even index, the untangling pass's roots exp(+2 pi i k / M) as [M / 4 + 1] float2)
  const int *sel;          // [n_sel]
  void *out;               // rows of the policy's element type
  long out_stride;
  int n, HH, M, D, n_taps, T, ld, n_out, n_sel, tiles;
  int lead;                // the call-relative index of the first output's last sample, 0 <= lead < D
  int tmod0;               // that sample's absolute time mod M
};

__device__ __forceinline__ float2 ch_sample(const short2 *p, int i) { const short2 v = p[i]; return make_float2((float)v.x, (float)v.y); }
__device__ __forceinline__ float2 ch_sample(const float2 *p, int i) { return p[i]; }
__device__ __forceinline__ float ch_sample(const short *p, int i) { return (float)p[i]; }
__device__ __forceinline__ float ch_sample(const float *p, int i) { return p[i]; }

// the input element decides the form: which side of ch_tile's `if constexpr` runs, and whether the tail is complex or real floats
template <class I> struct ChIn { static constexpr bool real = false; };
template <> struct ChIn<short> { static constexpr bool real = true; };
template <> struct ChIn<float> { static constexpr bool real = true; };

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

// the tail behind the call: the last HH samples of (tail, in[0 ... n)), every block its share — the blocks of a launch read
// the old buffer
template <class I>
__device__ __forceinline__ void ch_roll_tail(const ChArgs &a, int tid) {
  const I *in = static_cast<const I *>(a.in);
  for (int k = (int)blockIdx.x * CH_THREADS + tid; k < a.HH; k += (int)gridDim.x * CH_THREADS) {
    const int q = a.n + k;   // n < 2^30, HH < 2^18
    if constexpr (ChIn<I>::real)   // (a real row's tail: the floats at the head of the same buffers)
      reinterpret_cast<float *>(a.hist_new)[k] = q < a.HH ? reinterpret_cast<const float *>(a.hist)[q] : ch_sample(in, q - a.HH);
    else a.hist_new[k] = q < a.HH ? a.hist[q] : ch_sample(in, q - a.HH);
  }
}

// the untangling pass over Ti images of the H-point transforms Z of z[j] = w[2 j] + i w[2 j + 1], H = M / 2: lane (tt, k),
// k in [0, H / 2], takes the pair (k, kp = (H - k) mod H) in place, with a = Z[k], b = Z[kp], (c, s) = untw[k], in float32 and in
// this order (sdrhip_chanreal.h states it):
//     er = 0.5 (a.x + b.x)   ei = 0.5 (a.y - b.y)         E[k] = (Z[k] + conj Z[kp]) / 2
//     qr = 0.5 (a.y + b.y)   qi = 0.5 (b.x - a.x)         O[k] = (Z[k] - conj Z[kp]) / (2 i)
//     pr = fma(c, qr, -(s qi))   pi = fma(c, qi, s qr)    exp(+2 pi i k / M) O[k]
//     slot k  = (er + pr, ei + pi)
//     slot kp = (er - pr, pi - ei)     where kp != k; the lane of k = 0 writes it to slot H (y_H = Re E[0] - Re O[0])
// Slot H lies behind the transform's H elements, and no other lane reads or writes the pair's slots.
__device__ __forceinline__ void ch_untangle(const ChArgs &a, float2 *img, int Ti, int tid) {
  const int H = a.M >> 1, per = (H >> 1) + 1;
  const float2 *untw = reinterpret_cast<const float2 *>(a.invperm + ((H + 1) & ~1));
  for (int i = tid; i < Ti * per; i += CH_THREADS) {
    const int tt = i / per, k = i - tt * per, kp = k ? H - k : 0;
    float2 *z = img + tt * a.ld;
    const float2 va = z[k], vb = z[kp], w = untw[k];
    const float er = 0.5f * (va.x + vb.x), ei = 0.5f * (va.y - vb.y);
    const float qr = 0.5f * (va.y + vb.y), qi = 0.5f * (vb.x - va.x);
    const float pr = __builtin_fmaf(w.x, qr, -(w.y * qi)), pi = __builtin_fmaf(w.x, qi, w.y * qr);
    z[k] = make_float2(er + pr, ei + pi);
    if (kp != k || k == 0) z[k ? kp : H] = make_float2(er - pr, pi - ei);
  }
}

// the arguments an epilogue policy of a real row sees: M is the channels an image holds
__device__ __forceinline__ ChArgs ch_epi_args(const ChArgs &a) {
  ChArgs e = a;
  e.M = (a.M >> 1) + 1;
  return e;
}

// the LDS of a workgroup: the images (dynamic, the launch's) and a tile's time table, CH_TMAX + 1 entries each
struct ChLds { float2 *img; int *tmod, *rel; };
__device__ __forceinline__ ChLds ch_lds() {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  __shared__ int tmod_s[CH_TMAX + 1], rel_s[CH_TMAX + 1];
  return {reinterpret_cast<float2 *>(smem_raw), tmod_s, rel_s};
}

// one tile: phases 1 to 3 for the output times [tile T, tile T + Tc). A workgroup that walks several tiles calls this in a loop
// with nothing in between: the barrier behind a tile's time table also ends the store of the tile before (the images are written
// behind it), and the table itself is read in phase 1 only, which two barriers separate from the next tile's.
// A row of real samples (ChIn<I>::real): a.M is the definition's M, a.fft and a.invperm are the M / 2-point plan's, an image has
// M / 2 + 1 elements of a.ld.
template <class I, class E>
__device__ __forceinline__ void ch_tile(const ChArgs &a, const E &epi, int tile, const ChLds &lds, int tid) {
  constexpr bool real = ChIn<I>::real;
  const int M = a.M;
  const I *in = static_cast<const I *>(a.in);
  float2 *img = lds.img;
  const int j0 = tile * a.T, Tc = min(a.T, a.n_out - j0), halo = epi.halo(a, j0), Ti = Tc + halo;
  for (int tt = tid; tt < Ti; tt += CH_THREADS) {
    const long long jd = (long long)(j0 - halo + tt) * a.D;   // below n <= 2^30
    lds.tmod[tt] = (int)(((long long)a.tmod0 + jd) % M);
    lds.rel[tt] = a.lead + (int)jd;
  }
  __syncthreads();
  // phase 1
  for (int e = tid; e < Ti * M; e += CH_THREADS) {
    const int tt = e / M, r = e - tt * M;
    int rel = lds.rel[tt] - r;
    float re = 0.f, im = 0.f;   // (a real row: re alone)
#pragma unroll 4
    for (int l = r; l < a.n_taps; l += M, rel -= M) {
      // (the clamps never bind — see the head of the file; they keep a wrong count from becoming a wild read)
      if constexpr (real) {   // (the tail: the floats at the head of the same buffer)
        const float v = rel >= 0 ? ch_sample(in, min(rel, a.n - 1)) : reinterpret_cast<const float *>(a.hist)[max(a.HH + rel, 0)];
        re = __builtin_fmaf(a.taps[l], v, re);
      } else {
        const float2 v = rel >= 0 ? ch_sample(in, min(rel, a.n - 1)) : a.hist[max(a.HH + rel, 0)];
        const float hv = a.taps[l];
        re = __builtin_fmaf(hv, v.x, re);
        im = __builtin_fmaf(hv, v.y, im);
      }
    }
    int jw = r - lds.tmod[tt];
    jw += jw < 0 ? M : 0;
    if constexpr (real) reinterpret_cast<float *>(img)[2 * (tt * a.ld + a.invperm[jw >> 1]) + (jw & 1)] = re;
    else img[tt * a.ld + a.invperm[jw]] = make_float2(re, im);
  }
  __syncthreads();
  // phase 2
  int s = 1;
  for (int pass = a.fft.npass - 1; pass >= 0; pass--) {
    const int r = a.fft.radix[pass];
#define SDRHIP_CH_CALL(R_) ch_pass<R_>(img, a.fft, s, Ti, a.ld, tid)
    SDRHIP_GEN_RADIX_SWITCH(r, SDRHIP_CH_CALL)
#undef SDRHIP_CH_CALL
    __syncthreads();
    s *= r;
  }
  // phase 3
  if constexpr (real) {
    ch_untangle(a, img, Ti, tid);
    __syncthreads();
    epi.store(ch_epi_args(a), img, j0, Tc, halo, tid);
  } else epi.store(a, img, j0, Tc, halo, tid);
}

// every block, behind its tiles: the policy's roll on the arguments it sees
template <class I, class E>
__device__ __forceinline__ void ch_roll(const ChArgs &a, const E &epi, int tid) {
  if constexpr (ChIn<I>::real) epi.template roll<I>(ch_epi_args(a), tid);
  else epi.template roll<I>(a, tid);
}

// one tile per workgroup: tile blockIdx.x (not written as the walk at W = gridDim.x: compiled that way the row kernels took 190 to
// 203 VGPRs for their 79 to 81 — profiles/chan_body_refactor.md)
template <class I, class E>
__device__ __forceinline__ void ch_body(const ChArgs &a, const E &epi) {
  const ChLds lds = ch_lds();
  const int tid = (int)threadIdx.x, tile = (int)blockIdx.x;
  if (tile < a.tiles) ch_tile<I>(a, epi, tile, lds, tid);
  ch_roll<I>(a, epi, tid);
}

// a bounded walk of stride W: the first W workgroups of the launch's row take the tiles b, b + W, ... in that order and the others
// none; every workgroup rolls its share of the tail. W = gridDim.x is a launch of its own with fewer workgroups than tiles
// (chanpower.hip); a member of a group launch (sdrhip_changroup.h) passes the W of its own launch, whatever gridDim.x is.
template <class I, class E>
__device__ __forceinline__ void ch_body_walk(const ChArgs &a, const E &epi, int W) {
  const ChLds lds = ch_lds();
  const int tid = (int)threadIdx.x;
  if ((int)blockIdx.x < W)
    for (int tile = (int)blockIdx.x; tile < a.tiles; tile += W) ch_tile<I>(a, epi, tile, lds, tid);
  ch_roll<I>(a, epi, tid);
}

// the member table of a group launch, by value in the kernel arguments: workgroup (x, y) runs member y's body on m[y]. The
// index is blockIdx.y, so the pick is a scalar load from the argument segment.
constexpr int CG_MAX = SDRHIP_CHANGROUP_MAX;
constexpr size_t CG_ARG_BYTES = 4096;   // what a launch's argument segment may hold (eight ChAudioArgs are 2112 bytes)
template <class A>
struct ChGroupArgs { A m[CG_MAX]; };

// ---- host side: what the handle types hold and do ----------------------------------------------------------------------------
// the argument rules of create, in the header's order (before the context: host rules); h32: the taps rounded once to float32
// (real: the rules of sdrhip_chanreal.h — the type codes have the complex ones' values, M is even and at least 4, and the
// transform is M / 2 points long)
static inline void ch_require_args(int dtype, int M, int D, const double *taps, int n_taps, size_t max_in, std::vector<float> &h32,
                                   bool real = false) {
  SDRHIP_REQUIRE(dtype == SDRHIP_CHAN_CS16 || dtype == SDRHIP_CHAN_CF32, SDRHIP_E_INVALID, "bad dtype %d", dtype);
  const int m_min = real ? CH_M_MIN_REAL : CH_M_MIN;
  SDRHIP_REQUIRE(M >= m_min && M <= CH_M_MAX, SDRHIP_E_SIZE, "M %d outside [%d,%d] (one transform lives in one workgroup's LDS)", M,
                 m_min, CH_M_MAX);
  std::vector<int> radix;
  int bad = 1;
  if (real) {
    SDRHIP_REQUIRE(M % 2 == 0, SDRHIP_E_INVALID, "M %d is odd: a real row's transform is M / 2 points long", M);
    SDRHIP_REQUIRE(fftgen::GenPlan<float2>::factor(M / 2, radix, &bad), SDRHIP_E_INVALID,
                   "M / 2 = %d has the prime factor %d: the device transforms sizes made of 2, 3, 5, 7, 11 and 13", M / 2, bad);
  } else
    SDRHIP_REQUIRE(fftgen::GenPlan<float2>::factor(M, radix, &bad), SDRHIP_E_INVALID,
                   "M %d has the prime factor %d: the device transforms sizes made of 2, 3, 5, 7, 11 and 13", M, bad);
  SDRHIP_REQUIRE(D >= 1 && D <= M, SDRHIP_E_INVALID, "D %d outside [1,M = %d]", D, M);
  SDRHIP_REQUIRE(n_taps >= 1 && n_taps <= CH_BRANCH_MAX * M, SDRHIP_E_SIZE, "n_taps %d outside [1,%d M = %d]", n_taps, CH_BRANCH_MAX,
                 CH_BRANCH_MAX * M);
  require_max_in(max_in);
  h32.resize((size_t)n_taps);
  for (int i = 0; i < n_taps; i++) {
    h32[(size_t)i] = (float)taps[i];
    SDRHIP_REQUIRE(std::isfinite(h32[(size_t)i]), SDRHIP_E_INVALID, "tap %d is not finite as a float", i);
  }
}

struct ChPlan {
  sdrhip_ctx *ctx = nullptr;
  int dtype = SDRHIP_CHAN_CS16, M = 2, D = 1, n_taps = 1, T = 1, ld = 3, n_sel = 2;
  bool real = false;               // a row of real samples in (sdrhip_chanreal.h): the plan is M / 2 points long
  int nch = 2;                     // the channels: M, or M / 2 + 1 of a real row
  size_t max_in = 0;
  uint64_t consumed = 0;
  int cur = 0;                     // which tail buffer holds the state
  fftgen::GenPlan<float2> plan;
  DevBuf<float> taps;
  DevBuf<int> invperm, sel;
  std::vector<int> sel_host;       // [n_sel]
  DevBuf<float2> hist[2];          // [n_taps - 1] each (at least one element); a real row's tail is the floats at their head
  Staging stage;
  size_t in_elem() const { return (dtype == SDRHIP_CHAN_CS16 ? 4 : 8) / (real ? 2 : 1); }
  const char *nch_name() const { return real ? "K" : "M"; }
  int HH() const { return n_taps - 1; }
  size_t out_count(size_t n) const { return (size_t)((consumed + n) / (uint64_t)D - consumed / (uint64_t)D); }
  size_t out_count_max(size_t n) const { return ceil_div(n, (size_t)D); }   // whatever N is

  // inside make_handle, behind ch_require_args; the caller ends with allow_lds_max and its fresh state
  // A real row's plan (sdrhip_chanreal.h states the rule): the transform is L = M / 2 points long, an image holds the L + 1
  // channels at ld = (L + 1) | 1 elements — odd, so that consecutive images start two banks apart as the complex form's do —
  // and T is the complex form's: as many workgroups per call, each with half the LDS (twice the tile times in the same LDS
  // halve the workgroups of a call: a 2^21-sample call at M = 1024 then fills half the device and takes 1.6x as long).
  void build(sdrhip_ctx *c, int dtype_, int M_, int D_, const std::vector<float> &h32, size_t max_in_, bool real_ = false) {
    dtype = dtype_; M = M_; D = D_; n_taps = (int)h32.size(); max_in = max_in_; real = real_;
    const int L = real ? M / 2 : M;
    nch = real ? L + 1 : M;
    T = std::min(CH_TMAX, (M <= CH_M_SMALL ? CH_ELEMS_SMALL : CH_ELEMS_LARGE) / M);
    ld = real ? ((L + 1) | 1) : M + 1;
    plan.build(c, L, CH_M_MAX);
    // (a real row: the untangling pass's roots ride behind the permutation, at the next even index — ChArgs stays what it was)
    const size_t at = ((size_t)L + 1) & ~(size_t)1;
    std::vector<int> inv(real ? at + 2 * (size_t)(M / 4 + 1) : (size_t)L, 0);
    for (int pos = 0; pos < L; pos++) inv[(size_t)plan.perm[pos]] = pos;
    for (int k = 0; real && k <= M / 4; k++) {
      const double ph = 2.0 * 3.14159265358979323846 * (double)k / (double)M;
      const float w[2] = {(float)std::cos(ph), (float)std::sin(ph)};
      memcpy(&inv[at + 2 * (size_t)k], w, sizeof w);
    }
    invperm.alloc(inv.size());
    invperm.upload(inv.data(), inv.size(), c->stream);
    taps.alloc((size_t)n_taps);
    taps.upload(h32.data(), h32.size(), c->stream);
    sel.alloc((size_t)nch);
    select(nullptr, 0);
    for (auto &b : hist) { b.alloc((size_t)std::max(HH(), 1)); b.zero(c->stream); }
  }
  // set_channels: idx = NULL selects all nch in order; a bad selection changes nothing
  void select(const int *idx, int n) {
    std::vector<int> s;
    if (!idx) {
      s.resize((size_t)nch);
      for (int k = 0; k < nch; k++) s[(size_t)k] = k;
    } else {
      SDRHIP_REQUIRE(n >= 1 && n <= nch, SDRHIP_E_INVALID, "n_sel %d outside [1,%s = %d]", n, nch_name(), nch);
      std::vector<char> seen((size_t)nch, 0);
      for (int i = 0; i < n; i++) {
        SDRHIP_REQUIRE(idx[i] >= 0 && idx[i] < nch, SDRHIP_E_INVALID, "channel %d (row %d) outside [0,%d)", idx[i], i, nch);
        SDRHIP_REQUIRE(!seen[(size_t)idx[i]], SDRHIP_E_INVALID, "channel %d is selected twice (row %d)", idx[i], i);
        seen[(size_t)idx[i]] = 1;
      }
      s.assign(idx, idx + n);
    }
    put_sync(ctx, sel.p, s.data(), s.size() * sizeof(int));
    sel_host.swap(s);
    n_sel = (int)sel_host.size();
  }
  void set_taps(const double *t) {
    std::vector<float> h32((size_t)n_taps);
    for (int i = 0; i < n_taps; i++) {
      h32[(size_t)i] = (float)t[i];
      SDRHIP_REQUIRE(std::isfinite(h32[(size_t)i]), SDRHIP_E_INVALID, "tap %d is not finite as a float", i);
    }
    put_sync(ctx, taps.p, h32.data(), h32.size() * sizeof(float));
  }
  void fresh_tail() {
    SDRHIP_CHECK_HIP(hipMemsetAsync(hist[0].p, 0, hist[0].n * sizeof(float2), ctx->stream));
    SDRHIP_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    cur = 0; consumed = 0;
  }
  void get_tail(uint64_t *consumed_out, float *tail, size_t tail_len) {
    SDRHIP_REQUIRE(!tail || tail_len >= (size_t)HH(), SDRHIP_E_SIZE, "tail_len %zu < n_taps - 1 = %d", tail_len, HH());
    if (tail && HH() > 0 && !real) get_sync(ctx, tail, hist[cur].p, (size_t)HH() * sizeof(float2));
    if (tail && HH() > 0 && real) {   // (re, 0) pairs: one layout for the callers
      std::vector<float> re((size_t)HH());
      get_sync(ctx, re.data(), hist[cur].p, re.size() * sizeof(float));
      for (int i = 0; i < HH(); i++) { tail[2 * i] = re[(size_t)i]; tail[2 * i + 1] = 0.f; }
    }
    if (consumed_out) *consumed_out = consumed;
  }
  // the arguments of a launch of n >= 1 samples from the current state; the grid is max(tiles, 1) blocks of CH_THREADS
  ChArgs args(const void *in_dev, size_t n, void *out_dev, size_t out_stride, size_t n_out) const {
    ChArgs a;
    a.fft = plan.dev;
    a.in = in_dev; a.hist = hist[cur].p; a.hist_new = hist[cur ^ 1].p;
    a.taps = taps.p; a.invperm = invperm.p; a.sel = sel.p;
    a.out = out_dev; a.out_stride = (long)out_stride;
    a.n = (int)n; a.HH = HH(); a.M = M; a.D = D; a.n_taps = n_taps; a.T = T; a.ld = ld; a.n_out = (int)n_out; a.n_sel = n_sel;
    a.tiles = (int)ceil_div(n_out, (size_t)T);
    a.lead = (int)((uint64_t)D - 1 - consumed % (uint64_t)D);
    a.tmod0 = (int)((consumed + (uint64_t)a.lead) % (uint64_t)M);
    return a;
  }
  // the state moves on only behind a launch that was accepted
  void advance(size_t n) { consumed += n; cur ^= 1; }
  // a handle's entry of its [real][dtype] table of kernels or of their names
  template <class X>
  const X &pick(const X (&table)[2][2]) const { return table[real][dtype != SDRHIP_CHAN_CS16]; }
  // the launch of n >= 1 samples: max(blocks, 1) workgroups of CH_THREADS on the context's stream, with the state moved on
  // (always inlined: it is the tail of a handle type's launch(), and the library's dynamic symbols stay the handle types' own)
  template <class K, class... A>
  __attribute__((always_inline)) void launch_tiles(K kernel, int blocks, size_t lds, size_t n, const A &...a) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(kernel, dim3((unsigned)std::max(blocks, 1)), dim3(CH_THREADS), lds, ctx->stream, a...);
    SDRHIP_CHECK_HIP(hipGetLastError());
    advance(n);
  }
  // a handle type with state besides the tail has its own, and ends it with fresh_tail
  void fresh_state() { fresh_tail(); }
};

// ---- the entry points of a handle type H : ChPlan (channelizer.hip, chanaudio.hip, chanpower.hip) ---------------------------------
// H has kernel(), lds_bytes(), fresh_state() and, for the row calls, launch(in_dev, n, out_dev, out_stride, n_out).
// Both create calls of a type (real: sdrhip_chanreal.h's). rules(): the node's own argument rules, host rules like those before
// them; init(h): the node's own buffers, on the built plan.
template <class H, class Rules, class Init>
static inline int ch_create(sdrhip_ctx *ctx, int dtype, int M, int D, const double *taps, int n_taps, size_t max_in, H **out, bool real,
                            Rules &&rules, Init &&init) {
  return guarded([&] {
    if (out) *out = nullptr;
    SDRHIP_REQUIRE(out && taps, SDRHIP_E_INVALID, "NULL argument");
    std::vector<float> h32;
    ch_require_args(dtype, M, D, taps, n_taps, max_in, h32, real);
    rules();
    require_device_for_null_ctx(ctx);
    make_handle(ctx, out, true, [&](H *h) {
      h->build(ctx, dtype, M, D, h32, max_in, real);
      init(h);
      allow_lds_max(h->kernel(), h->lds_bytes());
      h->fresh_state();
    });
  });
}

template <class H>
static inline int ch_out_count(H *h, size_t n, size_t *n_out) {
  return guarded([&] {
    SDRHIP_REQUIRE(h && n_out, SDRHIP_E_INVALID, "NULL argument");
    *n_out = h->out_count(n);
  });
}

// the row calls: n_sel rows of elements of `ob` bytes; range: the call's name
template <class H>
static inline int ch_process_dev(H *h, const char *range, size_t ob, const void *in_dev, size_t n, void *out_dev, size_t out_stride,
                                 size_t *n_out) {
  return guarded([&] {
    Range roctx_range(range);
    if (n_out) *n_out = 0;
    if (!call_begin(h, "n", n, in_dev, out_dev)) return;
    const size_t no = h->out_count(n);
    const Strides s = call_strides("n", n, 0, no, out_stride, STRIDE_OUT);
    require_disjoint(in_dev, n, n, h->in_elem(), out_dev, s.out, no, ob, 1, (size_t)h->n_sel);
    h->launch(in_dev, n, out_dev, s.out, no);
    if (n_out) *n_out = no;
  });
}
template <class H>
static inline int ch_process(H *h, const char *range, size_t ob, const void *in_host, size_t n, void *out_host, size_t out_stride,
                             size_t *n_out) {
  return guarded([&] {
    Range roctx_range(range);
    if (n_out) *n_out = 0;
    if (!call_begin(h, "n", n, in_host, out_host)) return;
    const size_t no = h->out_count(n), rows = (size_t)h->n_sel, eb = h->in_elem();
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

template <class H>
static inline int ch_set_channels(H *h, const int *idx, int n_sel) {
  return guarded([&] {
    use_handle(h);
    h->select(idx, n_sel);
  });
}
template <class H>
static inline int ch_set_taps(H *h, const double *taps) {
  return guarded([&] {
    SDRHIP_REQUIRE(h && taps, SDRHIP_E_INVALID, "NULL argument");
    h->ctx->use();
    h->set_taps(taps);
  });
}
template <class H>
static inline int ch_reset(H *h) {
  return guarded([&] {
    use_handle(h);
    h->fresh_state();
  });
}
// the head of *_plan_info, inside the entry point's guarded(): the handle rule and the fields every type has
template <class H>
static inline void ch_plan_head(H *h, int *tile_times, int *branch_taps, int *lds_bytes) {
  SDRHIP_REQUIRE(h, SDRHIP_E_INVALID, "handle is NULL");
  if (tile_times) *tile_times = h->T;
  if (branch_taps) *branch_taps = (int)ceil_div((size_t)h->n_taps, (size_t)h->M);
  if (lds_bytes) *lds_bytes = (int)h->lds_bytes();
}
template <class H>
static inline int ch_kernel_names(H *h, char *buf, size_t len, const char *const (&names)[2][2]) {
  return guarded([&] {
    write_names(h, buf, len, [&] { return h->pick(names); });
  });
}

}  // namespace sdrhip

// ---- the channel group (sdrhip_changroup.h): borrowed handles of one type H : ChPlan behind one launch --------------------------
// One struct for the three families; what differs — the member type, its argument struct, its kernels — stands behind the
// two calls a family's create fills in (channelizer.hip, chanaudio.hip, chanpower.hip).
struct sdrhip_changroup {
  sdrhip_ctx *ctx = nullptr;
  int count = 0;
  sdrhip::ChPlan *member[sdrhip::CG_MAX] = {};   // the handles as H * (H derives from ChPlan alone)
  size_t lds = 0;                                // the launch's dynamic LDS: the largest member's
  int grid_x = 1;                                // plan_info's
  const char *names = "";
  // the row call and the power call of the family, inside the entry point's guarded(); NULL where the family has none
  void (*rows)(sdrhip_changroup *, const void *const *, const size_t *, void *const *, const size_t *, size_t *) = nullptr;
  void (*sums)(sdrhip_changroup *, const void *const *, const size_t *, double *const *, size_t *) = nullptr;
};

namespace sdrhip {

// a member's share of an accepted group call
struct CgCall { int i; size_t n, no, stride; };
struct CgExtent { uintptr_t b, e; };
static inline bool cg_meet(const CgExtent &a, const CgExtent &b) { return a.b < a.e && b.b < b.e && a.b < b.e && b.b < a.e; }
// the rule between members: no output over another member's input, nor over another member's output (a member's own pair is its
// own call's rule, checked before)
static inline void cg_require_disjoint(const CgCall *c, int na, const CgExtent *in, const CgExtent *out) {
  for (int a = 0; a < na; a++)
    for (int b = 0; b < na; b++) {
      if (a == b) continue;
      SDRHIP_REQUIRE(!cg_meet(out[a], in[b]), SDRHIP_E_INVALID, "the output range of member %d overlaps the input range of member %d", c[a].i,
                     c[b].i);
      SDRHIP_REQUIRE(a > b || !cg_meet(out[a], out[b]), SDRHIP_E_INVALID, "the output range of member %d overlaps the output range of member %d",
                     c[a].i, c[b].i);
    }
}

// The create calls' rules, in the header's order, and the handle. fill(g): the family's kernel limit, names and calls.
template <class H, class Fill>
static inline int cg_create(H *const *members, int count, sdrhip_changroup **out, Fill &&fill) {
  return guarded([&] {
    if (out) *out = nullptr;
    SDRHIP_REQUIRE(out && members, SDRHIP_E_INVALID, "NULL argument");
    SDRHIP_REQUIRE(count >= 1 && count <= CG_MAX, SDRHIP_E_SIZE, "count %d outside [1,%d]", count, CG_MAX);
    for (int i = 0; i < count; i++) SDRHIP_REQUIRE(members[i], SDRHIP_E_INVALID, "member %d is NULL", i);
    for (int i = 1; i < count; i++)
      for (int j = 0; j < i; j++) SDRHIP_REQUIRE(members[i] != members[j], SDRHIP_E_INVALID, "member %d is member %d again", i, j);
    for (int i = 1; i < count; i++)
      SDRHIP_REQUIRE(members[i]->ctx == members[0]->ctx, SDRHIP_E_INVALID, "member %d is on another context than member 0", i);
    for (int i = 1; i < count; i++)
      SDRHIP_REQUIRE(members[i]->dtype == members[0]->dtype && members[i]->real == members[0]->real, SDRHIP_E_INVALID,
                     "member %d has another input element type than member 0", i);
    make_handle(members[0]->ctx, out, true, [&](sdrhip_changroup *g) {
      g->count = count;
      for (int i = 0; i < count; i++) {
        g->member[i] = members[i];
        g->lds = std::max(g->lds, members[i]->lds_bytes());
      }
      fill(g);
    });
  });
}

// plan_info's grid_x of a family whose launch has a workgroup per tile
static inline int cg_grid_tiles(const sdrhip_changroup *g) {
  size_t gx = 1;
  for (int i = 0; i < g->count; i++) gx = std::max(gx, ceil_div(g->member[i]->out_count_max(g->member[i]->max_in), (size_t)g->member[i]->T));
  return (int)gx;
}

// A group call of a family of H, whose kernel takes the member table ChGroupArgs<A>: every member's own rules, then the rules
// between members, then ONE launch of dim3(grid.x, members in the call), and only behind it the members' states move on and n_out
// is set. `kernels`: the family's [real][dtype] table, picked at the launch. `pointers`: whether the family's further array
// arguments are all non-NULL — it joins in_dev and n in the one "NULL argument" rule, the first of the call, so that rule stands
// here once (a family without further arrays passes true). The family supplies
//   bool own(i, h, CgOwn &)     member i's own rules in its own call's order, first of them call_begin — false: n = 0, the member
//                               sits the call out — and what they leave: its outputs, its row stride, the bytes it writes
//   A    entry(h, call)         its entry of the table, from its state before the call (called once per accepted member)
//   int  grid(h, call, entry)   the workgroups its row of the grid needs
// -> the accepted calls, for what a family does behind the launch.
struct CgOwn { size_t no, stride; CgExtent out; };
struct CgCalls { CgCall c[CG_MAX]; int na = 0; };
template <class H, class A, class Own, class Entry, class Grid>
static inline CgCalls cg_call(sdrhip_changroup *g, void (*const (&kernels)[2][2])(const ChGroupArgs<A>), bool pointers,
                              const void *const *in_dev, const size_t *n, size_t *n_out, Own &&own, Entry &&entry, Grid &&grid) {
  SDRHIP_REQUIRE(in_dev && n && pointers, SDRHIP_E_INVALID, "NULL argument");
  for (int i = 0; n_out && i < g->count; i++) n_out[i] = 0;
  CgCalls r;
  CgCall *c = r.c;
  CgExtent in[CG_MAX], out[CG_MAX];
  int na = 0;
  for (int i = 0; i < g->count; i++) {
    H *h = static_cast<H *>(g->member[i]);
    CgOwn o;
    if (!own(i, h, o)) continue;
    in[na] = {(uintptr_t)in_dev[i], (uintptr_t)in_dev[i] + n[i] * h->in_elem()};
    out[na] = o.out;
    c[na++] = {i, n[i], o.no, o.stride};
  }
  cg_require_disjoint(c, na, in, out);
  if (!na) return r;
  g->ctx->use();
  ChGroupArgs<A> t;
  int gx = 1;
  for (int k = 0; k < na; k++) {
    H *h = static_cast<H *>(g->member[c[k].i]);
    t.m[k] = entry(h, c[k]);
    gx = std::max(gx, grid(h, c[k], t.m[k]));
  }
  for (int k = na; k < CG_MAX; k++) t.m[k] = t.m[0];   // (never read: grid.y is na)
  (void)hipGetLastError();
  hipLaunchKernelGGL(g->member[0]->pick(kernels), dim3((unsigned)gx, (unsigned)na), dim3(CH_THREADS), g->lds, g->ctx->stream, t);
  SDRHIP_CHECK_HIP(hipGetLastError());
  for (int k = 0; k < na; k++) {
    g->member[c[k].i]->advance(c[k].n);
    if (n_out) n_out[c[k].i] = c[k].no;
  }
  r.na = na;
  return r;
}

// The row call of a group of H with rows of `ob` bytes per element: a member's own rules are ch_process_dev's, in its order;
// table(h, in, out, call) is the member's entry of the kernel's table A; a workgroup per tile.
template <class H, class A, class Table>
static inline void cg_process_rows(sdrhip_changroup *g, void (*const (&kernels)[2][2])(const ChGroupArgs<A>), size_t ob,
                                   const void *const *in_dev, const size_t *n, void *const *out_dev, const size_t *out_stride,
                                   size_t *n_out, Table &&table) {
  cg_call<H>(
      g, kernels, out_dev && out_stride, in_dev, n, n_out,
      [&](int i, H *h, CgOwn &o) {
        if (!call_begin(h, "n", n[i], in_dev[i], out_dev[i])) return false;
        const size_t no = h->out_count(n[i]), rows = (size_t)h->n_sel;
        const Strides s = call_strides("n", n[i], 0, no, out_stride[i], STRIDE_OUT);
        require_disjoint(in_dev[i], n[i], n[i], h->in_elem(), out_dev[i], s.out, no, ob, 1, rows);
        o = {no, s.out, {(uintptr_t)out_dev[i], (uintptr_t)out_dev[i] + (no ? ((rows - 1) * s.out + no) * ob : 0)}};
        return true;
      },
      [&](H *h, const CgCall &c) { return table(h, in_dev[c.i], out_dev[c.i], c); },
      [](H *h, const CgCall &c, const A &) { return (int)ceil_div(c.no, (size_t)h->T); });
}

}  // namespace sdrhip
