// synthesis.hip — the polyphase synthesis bank (sdrhip_synthesis.h): channel rows to one wideband complex row interpolated by D,
// the channelizer's mirror. No reference node stands behind it; the header has the definition and the fast form. Two launches
// per call:
//   synthesis_transform_kernel   a workgroup of CH_THREADS lanes takes a tile of T consecutive columns (the channelizer's T and
//      image pitch):
//        1  all lanes: the images zeroed (skipped where every channel is selected: every element is then written in 2);
//        2  all lanes: element (i, tt) of the tile, tt fastest — row i's sample of column j0 + tt, T contiguous complex floats per
//           row (the mirror of the channelizer's transposed store) — written into image tt at the digit-reversed position of
//           channel sel[i], inverse_dit's input order;
//        3  all lanes: the backward decimation-in-time passes over the images at once — channelizer_body.hpp's ch_pass, which is
//           pass_dit's arithmetic with the lane loop over (image, butterfly);
//        4  all lanes: every v in natural order into its column of the ring.
//   synthesis_overlap_kernel     a lane per output time t: z[t] = sum_q g[q D + d] v_(m0 - q)[t mod M] as a float fma chain, q
//      ascending, the terms at q D + d >= n_taps skipped. Lanes run along t: a column is read contiguously in t mod M, the taps
//      contiguously in d.
// The column workspace is a ring of R = Q - 1 + max_in columns of M: the Q - 1 columns before the write position are the state
// (zeros at create and reset), a call writes its n <= max_in columns at the write position and the position moves on by n. The
// call's columns and the state's are disjoint ring slots, so the transform's blocks write nothing the overlap kernel of the
// call before still reads on the stream (launches are ordered) and nothing another block of their own launch reads; nothing is
// rolled behind a call.
// Reads stay inside in[row][0 ... n), the taps' n_taps, sel's n_sel, the permutation's M and the ring's R M elements: the index
// rules are beside each read. No atomics, no scratch.
#include "sdrhip_internal.hpp"
#include "sdrhip_synthesis.h"
#include "entry.hpp"
#include "channelizer_body.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

using namespace sdrhip;

namespace {

constexpr int SY_BRANCH_MAX = 64;                 // Q's bound
constexpr size_t SY_WS_MAX = size_t(1) << 28;     // the ring's elements: an element index is an int

struct SyArgs {
  fftgen::GenDev<float2> fft;
  const float2 *in;        // rows [n_sel][in_stride], n columns each
  long in_stride;
  float2 *ws;              // the ring [R][M]
  const float *taps;       // [n_taps]
  const int *invperm;      // [M] natural index -> position in inverse_dit's input
  const int *sel;          // [n_sel]
  float2 *out;             // [n D]
  int n, M, D, n_taps, T, ld, n_sel, R;
  int wpos;                // the ring slot of the call's first column, 0 <= wpos < R
  int tmod0;               // the call's first output time mod M
};

// ring slot of the call's column j, -R < j < R: wpos + j reduced once
__device__ __forceinline__ int sy_slot(const SyArgs &a, int j) {
  int c = a.wpos + j;
  c -= c >= a.R ? a.R : 0;
  c += c < 0 ? a.R : 0;
  return c;
}

__global__ __launch_bounds__(CH_THREADS) void synthesis_transform_kernel(const SyArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  float2 *img = reinterpret_cast<float2 *>(smem_raw);
  const int tid = (int)threadIdx.x, M = a.M;
  const int j0 = (int)blockIdx.x * a.T, Tc = min(a.T, a.n - j0);
  if (Tc <= 0) return;   // (uniform; the grid is ceil(n / T))
  if (a.n_sel < M) {
    for (int e = tid; e < Tc * a.ld; e += CH_THREADS) img[e] = make_float2(0.f, 0.f);
    __syncthreads();
  }
  // j0 + tt < n: inside the row; sel[i] in [0, M) (set_channels' rule), invperm a permutation of [0, M)
  for (int e = tid; e < a.n_sel * Tc; e += CH_THREADS) {
    const int i = e / Tc, tt = e - i * Tc;
    img[tt * a.ld + a.invperm[a.sel[i]]] = a.in[(long)i * a.in_stride + j0 + tt];
  }
  __syncthreads();
  int s = 1;
  for (int pass = a.fft.npass - 1; pass >= 0; pass--) {
    const int r = a.fft.radix[pass];
#define SDRHIP_SY_CALL(R_) ch_pass<R_>(img, a.fft, s, Tc, a.ld, tid)
    SDRHIP_GEN_RADIX_SWITCH(r, SDRHIP_SY_CALL)
#undef SDRHIP_SY_CALL
    __syncthreads();
    s *= r;
  }
  // column j0 + tt < n <= max_in <= R: one reduction; element slot M + j < R M <= 2^28
  for (int e = tid; e < Tc * M; e += CH_THREADS) {
    const int tt = e / M, j = e - tt * M;
    a.ws[sy_slot(a, j0 + tt) * M + j] = img[tt * a.ld + j];
  }
}

__global__ __launch_bounds__(CH_THREADS) void synthesis_overlap_kernel(const SyArgs a) {
  const int t = (int)blockIdx.x * CH_THREADS + (int)threadIdx.x;   // call-relative, n D < 2^30
  if (t >= a.n * a.D) return;
  const int m0 = t / a.D, d = t - m0 * a.D;
  const int tm = (a.tmod0 + t) % a.M;
  int c = sy_slot(a, m0);
  float re = 0.f, im = 0.f;
  // q < Q wherever q D + d < n_taps, so the walk goes back over at most Q - 1 slots: the state's
#pragma unroll 4
  for (int l = d; l < a.n_taps; l += a.D) {
    const float2 v = a.ws[c * a.M + tm];
    const float g = a.taps[l];
    re = __builtin_fmaf(g, v.x, re);
    im = __builtin_fmaf(g, v.y, im);
    c = c ? c - 1 : a.R - 1;
  }
  a.out[t] = make_float2(re, im);
}

constexpr const char *SY_NAMES = "synthesis_transform_kernel,synthesis_overlap_kernel";

// the taps rounded once to float32; a tap that is not finite as a float: SDRHIP_E_INVALID
std::vector<float> round_taps(const double *taps, int n_taps) {
  std::vector<float> g32((size_t)n_taps);
  for (int i = 0; i < n_taps; i++) {
    g32[(size_t)i] = (float)taps[i];
    SDRHIP_REQUIRE(std::isfinite(g32[(size_t)i]), SDRHIP_E_INVALID, "tap %d is not finite as a float", i);
  }
  return g32;
}

}  // namespace

struct sdrhip_synthesis {
  sdrhip_ctx *ctx = nullptr;
  int M = 2, D = 1, n_taps = 1, Q = 1, T = 1, ld = 3, n_sel = 2, R = 1;
  size_t max_in = 0;
  uint64_t consumed = 0;           // columns
  int wpos = 0;                    // the ring slot the next call's first column goes to
  fftgen::GenPlan<float2> plan;
  DevBuf<float> taps;
  DevBuf<int> invperm, sel;
  DevBuf<float2> ws;               // [R][M]
  Staging stage;
  size_t lds_bytes() const { return (size_t)T * (size_t)ld * sizeof(float2); }
  size_t state_elems() const { return (size_t)(Q - 1) * (size_t)M; }

  void build(sdrhip_ctx *c, int M_, int D_, const std::vector<float> &g32, size_t max_in_) {
    M = M_; D = D_; n_taps = (int)g32.size(); max_in = max_in_;
    Q = (int)ceil_div((size_t)n_taps, (size_t)D);
    R = Q - 1 + (int)max_in;
    T = std::min(CH_TMAX, (M <= CH_M_SMALL ? CH_ELEMS_SMALL : CH_ELEMS_LARGE) / M);
    ld = M + 1;
    plan.build(c, M, CH_M_MAX);
    std::vector<int> inv((size_t)M, 0);
    for (int pos = 0; pos < M; pos++) inv[(size_t)plan.perm[pos]] = pos;
    invperm.alloc(inv.size());
    invperm.upload(inv.data(), inv.size(), c->stream);
    taps.alloc((size_t)n_taps);
    taps.upload(g32.data(), g32.size(), c->stream);
    sel.alloc((size_t)M);
    select(nullptr, 0);
    ws.alloc((size_t)R * (size_t)M);
  }
  // set_channels: idx = NULL selects all M in order; a bad selection changes nothing (the channelizer's rules and messages,
  // restated: ChPlan::select is a member of the analysis plan)
  void select(const int *idx, int n) {
    std::vector<int> s;
    if (!idx) {
      s.resize((size_t)M);
      for (int k = 0; k < M; k++) s[(size_t)k] = k;
    } else {
      SDRHIP_REQUIRE(n >= 1 && n <= M, SDRHIP_E_INVALID, "n_sel %d outside [1,M = %d]", n, M);
      std::vector<char> seen((size_t)M, 0);
      for (int i = 0; i < n; i++) {
        SDRHIP_REQUIRE(idx[i] >= 0 && idx[i] < M, SDRHIP_E_INVALID, "channel %d (row %d) outside [0,%d)", idx[i], i, M);
        SDRHIP_REQUIRE(!seen[(size_t)idx[i]], SDRHIP_E_INVALID, "channel %d is selected twice (row %d)", idx[i], i);
        seen[(size_t)idx[i]] = 1;
      }
      s.assign(idx, idx + n);
    }
    put_sync(ctx, sel.p, s.data(), s.size() * sizeof(int));
    n_sel = (int)s.size();
  }
  // as freshly created: the state's Q - 1 columns at the ring's head, zeros
  void fresh_state() {
    if (Q > 1) SDRHIP_CHECK_HIP(hipMemsetAsync(ws.p, 0, state_elems() * sizeof(float2), ctx->stream));
    SDRHIP_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    wpos = (Q - 1) % R;
    consumed = 0;
  }
  // the state's columns, oldest first: the Q - 1 ring slots before wpos, in one piece or two
  void get_cols(float *cols) {
    const int first = (wpos - (Q - 1) + R) % R, head = std::min(Q - 1, R - first);
    get_sync(ctx, cols, ws.p + (size_t)first * (size_t)M, (size_t)head * (size_t)M * sizeof(float2));
    if (head < Q - 1) get_sync(ctx, cols + 2 * (size_t)head * (size_t)M, ws.p, (size_t)(Q - 1 - head) * (size_t)M * sizeof(float2));
  }
  // n >= 1 columns from the current state; the state moves on only behind launches that were accepted
  void launch(const void *in_dev, size_t n, size_t in_stride, void *out_dev) {
    ctx->use();
    SyArgs a;
    a.fft = plan.dev;
    a.in = static_cast<const float2 *>(in_dev); a.in_stride = (long)in_stride;
    a.ws = ws.p; a.taps = taps.p; a.invperm = invperm.p; a.sel = sel.p;
    a.out = static_cast<float2 *>(out_dev);
    a.n = (int)n; a.M = M; a.D = D; a.n_taps = n_taps; a.T = T; a.ld = ld; a.n_sel = n_sel; a.R = R;
    a.wpos = wpos;
    a.tmod0 = (int)((consumed % (uint64_t)M) * (uint64_t)D % (uint64_t)M);
    (void)hipGetLastError();
    hipLaunchKernelGGL(synthesis_transform_kernel, dim3((unsigned)ceil_div(n, (size_t)T)), dim3(CH_THREADS), lds_bytes(), ctx->stream, a);
    SDRHIP_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(synthesis_overlap_kernel, dim3((unsigned)ceil_div(n * (size_t)D, (size_t)CH_THREADS)), dim3(CH_THREADS), 0,
                       ctx->stream, a);
    SDRHIP_CHECK_HIP(hipGetLastError());
    consumed += n;
    wpos = (int)(((size_t)wpos + n) % (size_t)R);
  }
};

extern "C" {

int sdrhip_synthesis_create(sdrhip_ctx *ctx, int M, int D, const double *taps, int n_taps, size_t max_in, sdrhip_synthesis **out) {
  return guarded([&] {
    if (out) *out = nullptr;
    SDRHIP_REQUIRE(out && taps, SDRHIP_E_INVALID, "NULL argument");
    SDRHIP_REQUIRE(M >= CH_M_MIN && M <= CH_M_MAX, SDRHIP_E_SIZE, "M %d outside [%d,%d] (one transform lives in one workgroup's LDS)", M,
                   CH_M_MIN, CH_M_MAX);
    std::vector<int> radix;
    int bad = 1;
    SDRHIP_REQUIRE(fftgen::GenPlan<float2>::factor(M, radix, &bad), SDRHIP_E_INVALID,
                   "M %d has the prime factor %d: the device transforms sizes made of 2, 3, 5, 7, 11 and 13", M, bad);
    SDRHIP_REQUIRE(D >= 1 && D <= M, SDRHIP_E_INVALID, "D %d outside [1,M = %d]", D, M);
    SDRHIP_REQUIRE(n_taps >= 1 && n_taps <= SY_BRANCH_MAX * D, SDRHIP_E_SIZE, "n_taps %d outside [1,%d D = %d]", n_taps, SY_BRANCH_MAX,
                   SY_BRANCH_MAX * D);
    require_max_in(max_in);
    SDRHIP_REQUIRE(max_in * (size_t)D < (size_t(1) << 30), SDRHIP_E_SIZE, "max_in %zu x D %d: a call's %zu outputs are not below 2^30", max_in, D,
                   max_in * (size_t)D);
    const size_t Q = ceil_div((size_t)n_taps, (size_t)D);
    SDRHIP_REQUIRE((Q - 1 + max_in) * (size_t)M <= SY_WS_MAX, SDRHIP_E_SIZE,
                   "the column workspace (Q - 1 + max_in) M = (%zu + %zu) x %d exceeds 2^28 elements", Q - 1, max_in, M);
    const std::vector<float> g32 = round_taps(taps, n_taps);
    require_device_for_null_ctx(ctx);
    make_handle(ctx, out, true, [&](sdrhip_synthesis *h) {
      h->build(ctx, M, D, g32, max_in);
      allow_lds_max(synthesis_transform_kernel, h->lds_bytes());
      h->fresh_state();
    });
  });
}

int sdrhip_synthesis_out_count(sdrhip_synthesis *h, size_t n, size_t *n_out) {
  return guarded([&] {
    SDRHIP_REQUIRE(h && n_out, SDRHIP_E_INVALID, "NULL argument");
    *n_out = n * (size_t)h->D;
  });
}

int sdrhip_synthesis_process_dev(sdrhip_synthesis *h, const void *in_dev, size_t n, size_t in_stride, void *out_dev, size_t *n_out) {
  return guarded([&] {
    Range roctx_range("sdrhip_synthesis_process_dev");
    if (n_out) *n_out = 0;
    if (!call_begin(h, "n", n, in_dev, out_dev)) return;
    const size_t no = n * (size_t)h->D;
    const Strides s = call_strides("n", n, in_stride, no, 0, STRIDE_IN);
    require_disjoint(in_dev, s.in, n, sizeof(float2), out_dev, no, no, sizeof(float2), (size_t)h->n_sel, 1);
    h->launch(in_dev, n, s.in, out_dev);
    if (n_out) *n_out = no;
  });
}

int sdrhip_synthesis_process(sdrhip_synthesis *h, const void *in_host, size_t n, size_t in_stride, void *out_host, size_t *n_out) {
  return guarded([&] {
    Range roctx_range("sdrhip_synthesis_process");
    if (n_out) *n_out = 0;
    if (!call_begin(h, "n", n, in_host, out_host)) return;
    const size_t no = n * (size_t)h->D, rows = (size_t)h->n_sel, eb = sizeof(float2);
    const Strides s = call_strides("n", n, in_stride, no, 0, STRIDE_IN);
    // (the staged rows follow the selection: a set_channels can raise them)
    const size_t in_cap_b = rows * h->max_in * eb;
    if (h->stage.in.p && h->stage.in.n < in_cap_b) h->stage.in.alloc(in_cap_b);
    run_staged(h->ctx, h->stage, in_cap_b, h->max_in * (size_t)h->D * eb, {in_host, s.in * eb, n * eb, rows}, {out_host, no * eb, no * eb, 1},
               [&](void *in, void *out) {
                 h->launch(in, n, n, out);
                 return no * eb;
               });
    if (n_out) *n_out = no;
  });
}

int sdrhip_synthesis_set_channels(sdrhip_synthesis *h, const int *idx, int n_sel) {
  return guarded([&] {
    use_handle(h);
    h->select(idx, n_sel);
  });
}

int sdrhip_synthesis_set_taps(sdrhip_synthesis *h, const double *taps) {
  return guarded([&] {
    SDRHIP_REQUIRE(h && taps, SDRHIP_E_INVALID, "NULL argument");
    h->ctx->use();
    const std::vector<float> g32 = round_taps(taps, h->n_taps);
    put_sync(h->ctx, h->taps.p, g32.data(), g32.size() * sizeof(float));
  });
}

int sdrhip_synthesis_reset(sdrhip_synthesis *h) {
  return guarded([&] {
    use_handle(h);
    h->fresh_state();
  });
}

int sdrhip_synthesis_get_state(sdrhip_synthesis *h, uint64_t *consumed, float *cols, size_t cols_len) {
  return guarded([&] {
    use_handle(h);
    SDRHIP_REQUIRE(!cols || cols_len >= h->state_elems(), SDRHIP_E_SIZE, "cols_len %zu < (Q - 1) M = %zu", cols_len, h->state_elems());
    if (cols && h->Q > 1) h->get_cols(cols);
    if (consumed) *consumed = h->consumed;
  });
}

int sdrhip_synthesis_plan_info(sdrhip_synthesis *h, int *tile_times, int *branch_taps, int *lds_bytes, int *rows) {
  return guarded([&] {
    SDRHIP_REQUIRE(h, SDRHIP_E_INVALID, "handle is NULL");
    if (tile_times) *tile_times = h->T;
    if (branch_taps) *branch_taps = h->Q;
    if (lds_bytes) *lds_bytes = (int)h->lds_bytes();
    if (rows) *rows = h->n_sel;
  });
}

int sdrhip_synthesis_kernel_names(sdrhip_synthesis *h, char *buf, size_t len) {
  return guarded([&] {
    write_names(h, buf, len, [&] { return SY_NAMES; });
  });
}

int sdrhip_synthesis_destroy(sdrhip_synthesis *h) {
  return guarded([&] { destroy_handle(h); });
}

}  // extern "C"
