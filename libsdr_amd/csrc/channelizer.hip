// channelizer.hip — the polyphase channelizer (sdrhip_channelizer.h): one antenna row to M uniform channels decimated by D.
// No reference node stands behind it; the header has the definition and the fast form. The kernel body (phases 1 and 2: the
// branch sums into shifted, digit-reversed LDS images and the backward transform over all images of a tile at once) is
// channelizer_body.hpp's, which chanaudio.hip shares; this file's epilogue is
//   3  all lanes: the spectra transposed — row i gets the tile's T values of channel sel[i], contiguous; the images are one
//      element apart from a multiple of M in LDS so that the lanes of a row do not meet on a bank.
// Every block also rolls its share of the tail (the last n_taps - 1 samples, as complex float) into the handle's other tail
// buffer: the blocks of a launch read the old one.
// A handle of sdrhip_chanreal_channelizer_create (sdrhip_chanreal.h) runs channelizer_real_s16_kernel / channelizer_real_f32_kernel: the
// body's real form in front of the same epilogue, rows 0 ... M / 2.
// A group of handles (sdrhip_changroup.h) runs group_channelizer_*_kernel: the member table in the arguments, member blockIdx.y's
// body (ch_body: a workgroup per tile, as alone). Its row call is channelizer_body.hpp's cg_process_rows, a user of the one group
// call skeleton cg_call; the entry points every group has are at the end of this file.
#include "sdrhip_internal.hpp"
#include "sdrhip_channelizer.h"
#include "sdrhip_chanreal.h"
#include "entry.hpp"
#include "channelizer_body.hpp"

#include <algorithm>
#include <cmath>

using namespace sdrhip;

namespace {

static_assert(CH_TMAX <= CH_THREADS, "a tile's time table is made in one sweep of the lanes (a halo image takes a second)");

// complex float rows out, no image before the tile
struct ChStoreComplex {
  __device__ __forceinline__ int halo(const ChArgs &, int) const { return 0; }
  __device__ __forceinline__ void store(const ChArgs &a, const float2 *img, int j0, int Tc, int, int tid) const {
    float2 *out = static_cast<float2 *>(a.out);
    for (int e = tid; e < a.n_sel * Tc; e += CH_THREADS) {
      const int i = e / Tc, tt = e - i * Tc;
      out[(long)i * a.out_stride + j0 + tt] = img[tt * a.ld + a.sel[i]];
    }
  }
  template <class I>
  __device__ __forceinline__ void roll(const ChArgs &a, int tid) const { ch_roll_tail<I>(a, tid); }
};

__global__ __launch_bounds__(CH_THREADS) void channelizer_cs16_kernel(const ChArgs a) { ch_body<short2>(a, ChStoreComplex()); }
__global__ __launch_bounds__(CH_THREADS) void channelizer_cf32_kernel(const ChArgs a) { ch_body<float2>(a, ChStoreComplex()); }
__global__ __launch_bounds__(CH_THREADS) void channelizer_real_s16_kernel(const ChArgs a) { ch_body<short>(a, ChStoreComplex()); }
__global__ __launch_bounds__(CH_THREADS) void channelizer_real_f32_kernel(const ChArgs a) { ch_body<float>(a, ChStoreComplex()); }

// a group launch (sdrhip_changroup.h): member blockIdx.y's body on its own arguments
using CgArgs = ChGroupArgs<ChArgs>;
static_assert(sizeof(CgArgs) <= CG_ARG_BYTES, "the member table travels in the kernel arguments");
__global__ __launch_bounds__(CH_THREADS) void group_channelizer_cs16_kernel(const CgArgs g) { ch_body<short2>(g.m[blockIdx.y], ChStoreComplex()); }
__global__ __launch_bounds__(CH_THREADS) void group_channelizer_cf32_kernel(const CgArgs g) { ch_body<float2>(g.m[blockIdx.y], ChStoreComplex()); }
__global__ __launch_bounds__(CH_THREADS) void group_channelizer_real_s16_kernel(const CgArgs g) { ch_body<short>(g.m[blockIdx.y], ChStoreComplex()); }
__global__ __launch_bounds__(CH_THREADS) void group_channelizer_real_f32_kernel(const CgArgs g) { ch_body<float>(g.m[blockIdx.y], ChStoreComplex()); }

using ChKernel = void (*)(const ChArgs);
using CgKernel = void (*)(const CgArgs);
constexpr CgKernel CG_KERNELS[2][2] = {{group_channelizer_cs16_kernel, group_channelizer_cf32_kernel},
                                       {group_channelizer_real_s16_kernel, group_channelizer_real_f32_kernel}};
constexpr const char *CG_NAMES[2][2] = {{"group_channelizer_cs16_kernel", "group_channelizer_cf32_kernel"},
                                        {"group_channelizer_real_s16_kernel", "group_channelizer_real_f32_kernel"}};
constexpr ChKernel CH_KERNELS[2][2] = {{channelizer_cs16_kernel, channelizer_cf32_kernel}, {channelizer_real_s16_kernel, channelizer_real_f32_kernel}};
constexpr const char *CH_NAMES[2][2] = {{"channelizer_cs16_kernel", "channelizer_cf32_kernel"}, {"channelizer_real_s16_kernel", "channelizer_real_f32_kernel"}};

}  // namespace

struct sdrhip_channelizer : ChPlan {
  ChKernel kernel() const { return pick(CH_KERNELS); }
  size_t lds_bytes() const { return (size_t)T * (size_t)ld * sizeof(float2); }
  // n >= 1
  void launch(const void *in_dev, size_t n, void *out_dev, size_t out_stride, size_t n_out) {
    ctx->use();
    const ChArgs a = args(in_dev, n, out_dev, out_stride, n_out);
    launch_tiles(kernel(), a.tiles, lds_bytes(), n, a);
  }
};

namespace {

// both create calls; real: sdrhip_chanreal.h's
int create(sdrhip_ctx *ctx, int dtype, int M, int D, const double *taps, int n_taps, size_t max_in, sdrhip_channelizer **out, bool real) {
  return ch_create(ctx, dtype, M, D, taps, n_taps, max_in, out, real, [] {}, [](sdrhip_channelizer *) {});
}

// the row call of a channelizer group
void group_rows(sdrhip_changroup *g, const void *const *in_dev, const size_t *n, void *const *out_dev, const size_t *out_stride,
                size_t *n_out) {
  cg_process_rows<sdrhip_channelizer>(g, CG_KERNELS, sizeof(float2), in_dev, n, out_dev, out_stride, n_out,
                                      [](sdrhip_channelizer *h, const void *in, void *out, const CgCall &c) {
                                        return h->args(in, c.n, out, c.stride, c.no);
                                      });
}

}  // namespace

extern "C" {

int sdrhip_changroup_channelizer_create(sdrhip_channelizer *const *members, int count, sdrhip_changroup **out) {
  return cg_create(members, count, out, [](sdrhip_changroup *g) {
    allow_lds_max(g->member[0]->pick(CG_KERNELS), g->lds);
    g->grid_x = cg_grid_tiles(g);
    g->names = g->member[0]->pick(CG_NAMES);
    g->rows = group_rows;
  });
}

// the calls every group has; the family stands behind g->rows (the power call: chanpower.hip)
int sdrhip_changroup_process_dev(sdrhip_changroup *g, const void *const *in_dev, const size_t *n, void *const *out_dev,
                                 const size_t *out_stride, size_t *n_out) {
  return guarded([&] {
    Range roctx_range("sdrhip_changroup_process_dev");
    SDRHIP_REQUIRE(g, SDRHIP_E_INVALID, "handle is NULL");
    SDRHIP_REQUIRE(g->rows, SDRHIP_E_INVALID, "a power group has no rows: its call is sdrhip_changroup_power_process_dev");
    g->rows(g, in_dev, n, out_dev, out_stride, n_out);
  });
}

int sdrhip_changroup_plan_info(sdrhip_changroup *g, int *members, int *grid_x, int *lds_bytes) {
  return guarded([&] {
    SDRHIP_REQUIRE(g, SDRHIP_E_INVALID, "handle is NULL");
    if (members) *members = g->count;
    if (grid_x) *grid_x = g->grid_x;
    if (lds_bytes) *lds_bytes = (int)g->lds;
  });
}

int sdrhip_changroup_kernel_names(sdrhip_changroup *g, char *buf, size_t len) {
  return guarded([&] {
    write_names(g, buf, len, [&] { return g->names; });
  });
}

int sdrhip_changroup_destroy(sdrhip_changroup *g) {
  return guarded([&] { destroy_handle(g); });
}

int sdrhip_channelizer_create(sdrhip_ctx *ctx, int dtype, int M, int D, const double *taps, int n_taps, size_t max_in,
                              sdrhip_channelizer **out) {
  return create(ctx, dtype, M, D, taps, n_taps, max_in, out, false);
}

int sdrhip_chanreal_channelizer_create(sdrhip_ctx *ctx, int dtype, int M, int D, const double *taps, int n_taps, size_t max_in,
                                   sdrhip_channelizer **out) {
  return create(ctx, dtype, M, D, taps, n_taps, max_in, out, true);
}

int sdrhip_channelizer_out_count(sdrhip_channelizer *h, size_t n, size_t *n_out) { return ch_out_count(h, n, n_out); }

int sdrhip_channelizer_process_dev(sdrhip_channelizer *h, const void *in_dev, size_t n, void *out_dev, size_t out_stride, size_t *n_out) {
  return ch_process_dev(h, "sdrhip_channelizer_process_dev", sizeof(float2), in_dev, n, out_dev, out_stride, n_out);
}

int sdrhip_channelizer_process(sdrhip_channelizer *h, const void *in_host, size_t n, void *out_host, size_t out_stride, size_t *n_out) {
  return ch_process(h, "sdrhip_channelizer_process", sizeof(float2), in_host, n, out_host, out_stride, n_out);
}

int sdrhip_channelizer_set_channels(sdrhip_channelizer *h, const int *idx, int n_sel) { return ch_set_channels(h, idx, n_sel); }

int sdrhip_channelizer_set_taps(sdrhip_channelizer *h, const double *taps) { return ch_set_taps(h, taps); }

int sdrhip_channelizer_reset(sdrhip_channelizer *h) { return ch_reset(h); }

int sdrhip_channelizer_get_state(sdrhip_channelizer *h, uint64_t *consumed, float *tail, size_t tail_len) {
  return guarded([&] {
    use_handle(h);
    h->get_tail(consumed, tail, tail_len);
  });
}

int sdrhip_channelizer_plan_info(sdrhip_channelizer *h, int *tile_times, int *branch_taps, int *lds_bytes, int *rows) {
  return guarded([&] {
    ch_plan_head(h, tile_times, branch_taps, lds_bytes);
    if (rows) *rows = h->n_sel;
  });
}

int sdrhip_channelizer_kernel_names(sdrhip_channelizer *h, char *buf, size_t len) { return ch_kernel_names(h, buf, len, CH_NAMES); }

int sdrhip_channelizer_destroy(sdrhip_channelizer *h) {
  return guarded([&] { destroy_handle(h); });
}

}  // extern "C"
