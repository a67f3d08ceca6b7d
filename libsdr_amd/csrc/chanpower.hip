// chanpower.hip — the channel power monitor (sdrhip_chanpower.h): the polyphase channelizer's arithmetic on one antenna row with
// no rows out — M sums of |y|^2 per call, a smoothed level and a squelch flag per channel. Phases 1 and 2 are
// channelizer_body.hpp's, shared with channelizer.hip and chanaudio.hip, so the spectra have the plain channelizer's bits; this
// file's epilogue is
//   3  lane tid owns the channels k = tid, tid + CH_THREADS, ...: it walks the tile's images at img[tt ld + k] (consecutive
//      lanes read consecutive LDS words) and adds e = (double)re (double)re + (double)im (double)im, in time order, onto the
//      workgroup's row of the [grid][M] partial buffer — from +0 on the workgroup's first tile, a read-modify-write by the one
//      owner of the element on the later ones. No atomics: the order is the header's, whatever the timing.
// The grid is bounded (ch_body_walk at W = gridDim.x: workgroup b takes the tiles b, b + W, ...), so the partial buffer is. The
// finish step (cp_finish) runs behind the launch on the same stream, one lane per channel: the rows of the workgroups that ran,
// added in row order, the call's sum where asked for, and the level and flag update; calls, J and alpha come from the host as
// arguments.
// A handle of sdrhip_chanreal_power_create (sdrhip_chanreal.h) runs chanpower_real_s16_kernel / chanpower_real_f32_kernel: the body's real
// form in front of the same epilogue; the partial buffer, the finish launch and every per-channel array then take nch = M / 2 + 1
// channels.
// A group of handles (sdrhip_changroup.h) runs group_chanpower_*_kernel — the same walk with the member's own stride W, whatever
// the launch's gridDim.x — and group_chanpower_finish_kernel, the same finish step on member blockIdx.y's arguments.
#include "sdrhip_internal.hpp"
#include "sdrhip_chanpower.h"
#include "sdrhip_chanreal.h"
#include "entry.hpp"
#include "channelizer_body.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>

using namespace sdrhip;

namespace {

constexpr int CP_GRID_PER_CU = 2;   // (an M = 1024 workgroup's images take 64 KiB of the CU's 160; a real handle's take 32 KiB, and
                                    // its grid is kept at the same two per CU: the partial buffer and the finish launch grow with it)
constexpr int CP_BATCH = 32;        // partial rows the finish kernel has in flight per lane

// no rows out, no image before the tile; `partial` is [gridDim.x][nch]
struct ChStorePower {
  double *partial;
  __device__ __forceinline__ int halo(const ChArgs &, int) const { return 0; }
  __device__ __forceinline__ void store(const ChArgs &a, const float2 *img, int j0, int Tc, int, int tid) const {
    double *row = partial + (size_t)blockIdx.x * (size_t)a.M;
    const bool first = j0 == (int)blockIdx.x * a.T;   // the workgroup's first tile is tile blockIdx.x
    for (int k = tid; k < a.M; k += CH_THREADS) {
      double acc = first ? 0.0 : row[k];
#pragma unroll 4
      for (int tt = 0; tt < Tc; tt++) {
        const float2 y = img[tt * a.ld + k];
        const double re = (double)y.x, im = (double)y.y;
        acc += re * re + im * im;   // (-ffp-contract=off: two exact products, one rounded add, one rounded accumulation)
      }
      row[k] = acc;
    }
  }
  template <class I>
  __device__ __forceinline__ void roll(const ChArgs &a, int tid) const { ch_roll_tail<I>(a, tid); }
};

__global__ __launch_bounds__(CH_THREADS) void chanpower_cs16_kernel(const ChArgs a, double *partial) {
  ch_body_walk<short2>(a, ChStorePower{partial}, (int)gridDim.x);
}
__global__ __launch_bounds__(CH_THREADS) void chanpower_cf32_kernel(const ChArgs a, double *partial) {
  ch_body_walk<float2>(a, ChStorePower{partial}, (int)gridDim.x);
}
__global__ __launch_bounds__(CH_THREADS) void chanpower_real_s16_kernel(const ChArgs a, double *partial) {
  ch_body_walk<short>(a, ChStorePower{partial}, (int)gridDim.x);
}
__global__ __launch_bounds__(CH_THREADS) void chanpower_real_f32_kernel(const ChArgs a, double *partial) {
  ch_body_walk<float>(a, ChStorePower{partial}, (int)gridDim.x);
}

using CpKernel = void (*)(const ChArgs, double *);
constexpr CpKernel CP_KERNELS[2][2] = {{chanpower_cs16_kernel, chanpower_cf32_kernel}, {chanpower_real_s16_kernel, chanpower_real_f32_kernel}};
constexpr const char *CP_NAMES[2][2] = {{"chanpower_cs16_kernel,chanpower_finish_kernel", "chanpower_cf32_kernel,chanpower_finish_kernel"},
                                        {"chanpower_real_s16_kernel,chanpower_finish_kernel", "chanpower_real_f32_kernel,chanpower_finish_kernel"}};

struct CpFinishArgs {
  const double *partial;            // [rows][M]
  const double *open_thr, *close_thr;   // [M]
  double *level;                    // [M]
  unsigned char *open;              // [M]
  double *sum;                      // [M] or NULL
  double alpha;
  int M, rows, J, first;            // M: the handle's channels (nch); rows: the workgroups that ran (0 where J = 0); first: calls == 0
};

// the finish step of one handle, one lane per channel (by value: the two kernels below hand it their own copy of the arguments)
__device__ __forceinline__ void cp_finish(const CpFinishArgs f) {
  const int k = (int)blockIdx.x * CH_THREADS + (int)threadIdx.x;
  if (k >= f.M) return;
  // the rows in increasing order, CP_BATCH loads in flight at a time: the adds are a chain, the loads need not wait for it
  const double *col = f.partial + k;
  double s = 0.0;
  int b = 0;
  for (; b + CP_BATCH <= f.rows; b += CP_BATCH) {
    double v[CP_BATCH];
#pragma unroll
    for (int i = 0; i < CP_BATCH; i++) v[i] = col[(size_t)(b + i) * (size_t)f.M];
#pragma unroll
    for (int i = 0; i < CP_BATCH; i++) s += v[i];
  }
  for (; b < f.rows; b++) s += col[(size_t)b * (size_t)f.M];
  if (f.sum) f.sum[k] = s;
  if (f.J <= 0) return;
  const double mean = s / (double)f.J, old = f.level[k];
  const double level = f.first ? mean : old + f.alpha * (mean - old);
  f.level[k] = level;
  f.open[k] = f.open[k] ? !(level < f.close_thr[k]) : level >= f.open_thr[k];
}

__global__ __launch_bounds__(CH_THREADS) void chanpower_finish_kernel(const CpFinishArgs f) { cp_finish(f); }

// A group launch (sdrhip_changroup.h): member blockIdx.y's body on its own arguments. W is the stride of the member's own launch,
// min(tiles, G): the first W workgroups of the row walk the tiles as that launch's would, each on its own row of the member's
// partial buffer, so the finish step adds the same rows in the same order.
struct CpGroupMember {
  ChArgs a;
  double *partial;   // [G][nch], the member's
  int W;
};
using CpGroupArgs = ChGroupArgs<CpGroupMember>;
using CpGroupFinishArgs = ChGroupArgs<CpFinishArgs>;
static_assert(sizeof(CpGroupArgs) <= CG_ARG_BYTES && sizeof(CpGroupFinishArgs) <= CG_ARG_BYTES, "the member table travels in the kernel arguments");

__global__ __launch_bounds__(CH_THREADS) void group_chanpower_cs16_kernel(const CpGroupArgs g) {
  const CpGroupMember &m = g.m[blockIdx.y];
  ch_body_walk<short2>(m.a, ChStorePower{m.partial}, m.W);
}
__global__ __launch_bounds__(CH_THREADS) void group_chanpower_cf32_kernel(const CpGroupArgs g) {
  const CpGroupMember &m = g.m[blockIdx.y];
  ch_body_walk<float2>(m.a, ChStorePower{m.partial}, m.W);
}
__global__ __launch_bounds__(CH_THREADS) void group_chanpower_real_s16_kernel(const CpGroupArgs g) {
  const CpGroupMember &m = g.m[blockIdx.y];
  ch_body_walk<short>(m.a, ChStorePower{m.partial}, m.W);
}
__global__ __launch_bounds__(CH_THREADS) void group_chanpower_real_f32_kernel(const CpGroupArgs g) {
  const CpGroupMember &m = g.m[blockIdx.y];
  ch_body_walk<float>(m.a, ChStorePower{m.partial}, m.W);
}

// member blockIdx.y's finish step: the same adds in the same order, the same level and flag step
__global__ __launch_bounds__(CH_THREADS) void group_chanpower_finish_kernel(const CpGroupFinishArgs g) { cp_finish(g.m[blockIdx.y]); }

using CpGroupKernel = void (*)(const CpGroupArgs);
constexpr CpGroupKernel CPG_KERNELS[2][2] = {{group_chanpower_cs16_kernel, group_chanpower_cf32_kernel},
                                             {group_chanpower_real_s16_kernel, group_chanpower_real_f32_kernel}};
constexpr const char *CPG_NAMES[2][2] = {
    {"group_chanpower_cs16_kernel,group_chanpower_finish_kernel", "group_chanpower_cf32_kernel,group_chanpower_finish_kernel"},
    {"group_chanpower_real_s16_kernel,group_chanpower_finish_kernel", "group_chanpower_real_f32_kernel,group_chanpower_finish_kernel"}};

void require_alpha(double alpha) {
  SDRHIP_REQUIRE(alpha > 0.0 && alpha <= 1.0, SDRHIP_E_INVALID, "alpha %g outside (0,1]", alpha);   // (a NaN fails both)
}

}  // namespace

struct sdrhip_chanpower : ChPlan {
  double alpha = 1.0;
  uint64_t calls = 0;
  int G = 1;                                   // the workgroups of a launch at most
  DevBuf<double> partial, level, thr_open, thr_close;   // [G][nch], [nch], [nch], [nch]
  DevBuf<unsigned char> open;                  // [nch]
  CpKernel kernel() const { return pick(CP_KERNELS); }
  size_t lds_bytes() const { return (size_t)T * (size_t)ld * sizeof(float2); }
  void fresh_state() {
    SDRHIP_CHECK_HIP(hipMemsetAsync(level.p, 0, (size_t)nch * sizeof(double), ctx->stream));
    SDRHIP_CHECK_HIP(hipMemsetAsync(open.p, 0, (size_t)nch, ctx->stream));
    fresh_tail();   // (synchronises)
    calls = 0;
  }
  // the finish step's arguments behind a main launch of `rows` workgroups
  CpFinishArgs finish_args(double *sum_dev, int rows, size_t n_out) const {
    CpFinishArgs f;
    f.partial = partial.p; f.open_thr = thr_open.p; f.close_thr = thr_close.p; f.level = level.p; f.open = open.p; f.sum = sum_dev;
    f.alpha = alpha; f.M = nch; f.rows = rows; f.J = (int)n_out; f.first = calls == 0;
    return f;
  }
  // n >= 1; sum_dev may be NULL
  void launch(const void *in_dev, size_t n, double *sum_dev, size_t n_out) {
    ctx->use();
    const ChArgs a = args(in_dev, n, nullptr, 0, n_out);
    const int rows = std::min(a.tiles, G);
    launch_tiles(kernel(), rows, lds_bytes(), n, a, partial.p);
    if (n_out == 0 && !sum_dev) return;
    const CpFinishArgs f = finish_args(sum_dev, rows, n_out);
    hipLaunchKernelGGL(chanpower_finish_kernel, dim3((unsigned)ceil_div((size_t)nch, (size_t)CH_THREADS)), dim3(CH_THREADS), 0, ctx->stream, f);
    SDRHIP_CHECK_HIP(hipGetLastError());
    if (n_out) calls++;
  }
};

namespace {

// both create calls; real: sdrhip_chanreal.h's
int create(sdrhip_ctx *ctx, int dtype, int M, int D, const double *taps, int n_taps, size_t max_in, double alpha, sdrhip_chanpower **out,
           bool real) {
  return ch_create(ctx, dtype, M, D, taps, n_taps, max_in, out, real, [&] { require_alpha(alpha); }, [&](sdrhip_chanpower *h) {
    const size_t K = (size_t)h->nch;
    h->alpha = alpha;
    const char *e = getenv("SDRHIP_CHANPOWER_GRID");   // read once: the partial buffer is allocated for it
    h->G = std::max(1, CP_GRID_PER_CU * ctx->prop.multiProcessorCount);
    if (e && atoi(e) >= 1) h->G = std::min(h->G, atoi(e));
    // (no call has more tiles than max_in gives)
    h->G = (int)std::min((size_t)h->G, std::max(ceil_div(h->out_count_max(max_in), (size_t)h->T), (size_t)1));
    h->partial.alloc((size_t)h->G * K);
    h->level.alloc(K);
    h->open.alloc(K);
    std::vector<double> inf(K, HUGE_VAL), zero(K, 0.0);
    h->thr_open.alloc(K);
    h->thr_open.upload(inf.data(), inf.size(), ctx->stream);
    h->thr_close.alloc(K);
    h->thr_close.upload(zero.data(), zero.size(), ctx->stream);
    SDRHIP_CHECK_HIP(hipStreamSynchronize(ctx->stream));   // (the uploads read locals)
  });
}

// The call of a power group (cg_call): a member's own rules are sdrhip_chanpower_process_dev's, in its order; behind the main launch
// and the members' states, the finish launch over the members whose own call would have one.
void group_sums(sdrhip_changroup *g, const void *const *in_dev, const size_t *n, double *const *sum_dev, size_t *n_out) {
  using H = sdrhip_chanpower;
  const auto sum_of = [&](int i) { return sum_dev ? sum_dev[i] : nullptr; };
  const auto walk_of = [](const H *h, size_t no) { return std::min((int)ceil_div(no, (size_t)h->T), h->G); };   // launch()'s `rows`
  const CgCalls r = cg_call<H>(
      g, CPG_KERNELS, true, in_dev, n, n_out,
      [&](int i, H *h, CgOwn &o) {
        double *sum = sum_of(i);
        if (!call_begin(h, "n", n[i], in_dev[i], sum ? (const void *)sum : in_dev[i])) return false;
        if (sum) require_disjoint(in_dev[i], n[i], n[i], h->in_elem(), sum, (size_t)h->nch, (size_t)h->nch, sizeof(double), 1);
        o = {h->out_count(n[i]), 0, {(uintptr_t)sum, (uintptr_t)sum + (sum ? (size_t)h->nch * sizeof(double) : 0)}};
        return true;
      },
      [&](H *h, const CgCall &c) { return CpGroupMember{h->args(in_dev[c.i], c.n, nullptr, 0, c.no), h->partial.p, walk_of(h, c.no)}; },
      [](H *, const CgCall &, const CpGroupMember &m) { return m.W; });
  // the finish table: the members whose own call would have that step (finish_args reads `calls`, which moves only below)
  CpGroupFinishArgs ft;
  int fx = 1, nf = 0;
  for (int k = 0; k < r.na; k++) {
    const CgCall &c = r.c[k];
    H *h = static_cast<H *>(g->member[c.i]);
    if (c.no == 0 && !sum_of(c.i)) continue;
    ft.m[nf++] = h->finish_args(sum_of(c.i), walk_of(h, c.no), c.no);
    fx = std::max(fx, (int)ceil_div((size_t)h->nch, (size_t)CH_THREADS));
  }
  if (!nf) return;
  for (int k = nf; k < CG_MAX; k++) ft.m[k] = ft.m[0];
  hipLaunchKernelGGL(group_chanpower_finish_kernel, dim3((unsigned)fx, (unsigned)nf), dim3(CH_THREADS), 0, g->ctx->stream, ft);
  SDRHIP_CHECK_HIP(hipGetLastError());
  for (int k = 0; k < r.na; k++)
    if (r.c[k].no) static_cast<H *>(g->member[r.c[k].i])->calls++;
}

}  // namespace

extern "C" {

int sdrhip_changroup_power_create(sdrhip_chanpower *const *members, int count, sdrhip_changroup **out) {
  return cg_create(members, count, out, [](sdrhip_changroup *g) {
    allow_lds_max(g->member[0]->pick(CPG_KERNELS), g->lds);
    for (int i = 0; i < g->count; i++) g->grid_x = std::max(g->grid_x, static_cast<sdrhip_chanpower *>(g->member[i])->G);
    g->names = g->member[0]->pick(CPG_NAMES);
    g->sums = group_sums;
  });
}

int sdrhip_changroup_power_process_dev(sdrhip_changroup *g, const void *const *in_dev, const size_t *n, double *const *sum_dev,
                                       size_t *n_out) {
  return guarded([&] {
    Range roctx_range("sdrhip_changroup_power_process_dev");
    SDRHIP_REQUIRE(g, SDRHIP_E_INVALID, "handle is NULL");
    SDRHIP_REQUIRE(g->sums, SDRHIP_E_INVALID, "not a power group: its call is sdrhip_changroup_process_dev");
    g->sums(g, in_dev, n, sum_dev, n_out);
  });
}

int sdrhip_chanpower_create(sdrhip_ctx *ctx, int dtype, int M, int D, const double *taps, int n_taps, size_t max_in, double alpha,
                            sdrhip_chanpower **out) {
  return create(ctx, dtype, M, D, taps, n_taps, max_in, alpha, out, false);
}

int sdrhip_chanreal_power_create(sdrhip_ctx *ctx, int dtype, int M, int D, const double *taps, int n_taps, size_t max_in, double alpha,
                                 sdrhip_chanpower **out) {
  return create(ctx, dtype, M, D, taps, n_taps, max_in, alpha, out, true);
}

int sdrhip_chanpower_out_count(sdrhip_chanpower *h, size_t n, size_t *n_out) { return ch_out_count(h, n, n_out); }

int sdrhip_chanpower_process_dev(sdrhip_chanpower *h, const void *in_dev, size_t n, double *sum_dev, size_t *n_out) {
  return guarded([&] {
    Range roctx_range("sdrhip_chanpower_process_dev");
    if (n_out) *n_out = 0;
    if (!call_begin(h, "n", n, in_dev, sum_dev ? (const void *)sum_dev : in_dev)) return;   // (the sums are optional)
    const size_t no = h->out_count(n);
    if (sum_dev) require_disjoint(in_dev, n, n, h->in_elem(), sum_dev, (size_t)h->nch, (size_t)h->nch, sizeof(double), 1);
    h->launch(in_dev, n, sum_dev, no);
    if (n_out) *n_out = no;
  });
}

int sdrhip_chanpower_process(sdrhip_chanpower *h, const void *in_host, size_t n, double *sum_host, size_t *n_out) {
  return guarded([&] {
    Range roctx_range("sdrhip_chanpower_process");
    if (n_out) *n_out = 0;
    if (!call_begin(h, "n", n, in_host, sum_host)) return;
    const size_t no = h->out_count(n), eb = h->in_elem(), row_b = (size_t)h->nch * sizeof(double);
    run_staged(h->ctx, h->stage, h->max_in * eb, row_b, {in_host, n * eb, n * eb, 1}, {sum_host, row_b, row_b, 1},
               [&](void *in, void *out) {
                 h->launch(in, n, static_cast<double *>(out), no);
                 return row_b;
               });
    if (n_out) *n_out = no;
  });
}

int sdrhip_chanpower_set_thresholds(sdrhip_chanpower *h, const double *open_thr, const double *close_thr) {
  return guarded([&] {
    SDRHIP_REQUIRE(h && open_thr && close_thr, SDRHIP_E_INVALID, "NULL argument");
    for (int k = 0; k < h->nch; k++)   // (a NaN fails the comparison it meets)
      SDRHIP_REQUIRE(close_thr[k] >= 0.0 && close_thr[k] <= open_thr[k], SDRHIP_E_INVALID,
                     "thresholds of channel %d: 0 <= close_thr %g <= open_thr %g does not hold", k, close_thr[k], open_thr[k]);
    h->ctx->use();
    // stream-ordered after the launches already enqueued; both or none is not promised on a failing device
    const size_t b = (size_t)h->nch * sizeof(double);
    put_sync(h->ctx, h->thr_open.p, open_thr, b);
    put_sync(h->ctx, h->thr_close.p, close_thr, b);
  });
}

int sdrhip_chanpower_set_alpha(sdrhip_chanpower *h, double alpha) {
  return guarded([&] {
    SDRHIP_REQUIRE(h, SDRHIP_E_INVALID, "handle is NULL");
    require_alpha(alpha);
    h->alpha = alpha;
  });
}

int sdrhip_chanpower_set_taps(sdrhip_chanpower *h, const double *taps) { return ch_set_taps(h, taps); }

int sdrhip_chanpower_reset(sdrhip_chanpower *h) { return ch_reset(h); }

int sdrhip_chanpower_get_levels(sdrhip_chanpower *h, double *level, unsigned char *open, int len) {
  return guarded([&] {
    use_handle(h);
    SDRHIP_REQUIRE(len >= h->nch, SDRHIP_E_SIZE, "len %d < %s = %d", len, h->nch_name(), h->nch);
    if (level) get_sync(h->ctx, level, h->level.p, (size_t)h->nch * sizeof(double));
    if (open) get_sync(h->ctx, open, h->open.p, (size_t)h->nch);
  });
}

int sdrhip_chanpower_get_occupied(sdrhip_chanpower *h, int *idx, int cap, int *count) {
  return guarded([&] {
    use_handle(h);
    SDRHIP_REQUIRE(count && (idx || cap <= 0), SDRHIP_E_INVALID, "NULL argument");
    std::vector<unsigned char> open((size_t)h->nch);
    get_sync(h->ctx, open.data(), h->open.p, open.size());
    int n = 0;
    for (int k = 0; k < h->nch; k++)
      if (open[(size_t)k]) {
        if (n < cap) idx[n] = k;
        n++;
      }
    *count = n;
  });
}

int sdrhip_chanpower_get_state(sdrhip_chanpower *h, uint64_t *consumed, float *tail, size_t tail_len, uint64_t *calls) {
  return guarded([&] {
    use_handle(h);
    h->get_tail(consumed, tail, tail_len);
    if (calls) *calls = h->calls;
  });
}

int sdrhip_chanpower_plan_info(sdrhip_chanpower *h, int *tile_times, int *branch_taps, int *lds_bytes, int *grid, int *partial_bytes) {
  return guarded([&] {
    ch_plan_head(h, tile_times, branch_taps, lds_bytes);
    if (grid) *grid = h->G;
    if (partial_bytes) *partial_bytes = (int)(h->partial.n * sizeof(double));
  });
}

int sdrhip_chanpower_kernel_names(sdrhip_chanpower *h, char *buf, size_t len) { return ch_kernel_names(h, buf, len, CP_NAMES); }

int sdrhip_chanpower_destroy(sdrhip_chanpower *h) {
  return guarded([&] { destroy_handle(h); });
}

}  // extern "C"
