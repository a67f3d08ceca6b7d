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

using ChKernel = void (*)(const ChArgs);
constexpr ChKernel CH_KERNELS[2][2] = {{channelizer_cs16_kernel, channelizer_cf32_kernel}, {channelizer_real_s16_kernel, channelizer_real_f32_kernel}};
constexpr const char *CH_NAMES[2][2] = {{"channelizer_cs16_kernel", "channelizer_cf32_kernel"}, {"channelizer_real_s16_kernel", "channelizer_real_f32_kernel"}};

}  // namespace

struct sdrhip_channelizer : ChPlan {
  ChKernel kernel() const { return CH_KERNELS[real][dtype != SDRHIP_CHAN_CS16]; }
  size_t lds_bytes() const { return (size_t)T * (size_t)ld * sizeof(float2); }
  // n >= 1
  void launch(const void *in_dev, size_t n, void *out_dev, size_t out_stride, size_t n_out) {
    ctx->use();
    const ChArgs a = args(in_dev, n, out_dev, out_stride, n_out);
    const dim3 grid((unsigned)std::max(a.tiles, 1)), block(CH_THREADS);
    const size_t lds = lds_bytes();
    (void)hipGetLastError();
    hipLaunchKernelGGL(kernel(), grid, block, lds, ctx->stream, a);
    SDRHIP_CHECK_HIP(hipGetLastError());
    advance(n);
  }
};

namespace {

// both create calls; real: sdrhip_chanreal.h's
int create(sdrhip_ctx *ctx, int dtype, int M, int D, const double *taps, int n_taps, size_t max_in, sdrhip_channelizer **out, bool real) {
  return guarded([&] {
    if (out) *out = nullptr;
    SDRHIP_REQUIRE(out && taps, SDRHIP_E_INVALID, "NULL argument");
    std::vector<float> h32;
    ch_require_args(dtype, M, D, taps, n_taps, max_in, h32, real);
    require_device_for_null_ctx(ctx);
    make_handle(ctx, out, true, [&](sdrhip_channelizer *h) {
      h->build(ctx, dtype, M, D, h32, max_in, real);
      allow_lds_max(h->kernel(), h->lds_bytes());
      h->fresh_tail();
    });
  });
}

}  // namespace

extern "C" {

int sdrhip_channelizer_create(sdrhip_ctx *ctx, int dtype, int M, int D, const double *taps, int n_taps, size_t max_in,
                              sdrhip_channelizer **out) {
  return create(ctx, dtype, M, D, taps, n_taps, max_in, out, false);
}

int sdrhip_chanreal_channelizer_create(sdrhip_ctx *ctx, int dtype, int M, int D, const double *taps, int n_taps, size_t max_in,
                                   sdrhip_channelizer **out) {
  return create(ctx, dtype, M, D, taps, n_taps, max_in, out, true);
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
    h->select(idx, n_sel);
  });
}

int sdrhip_channelizer_set_taps(sdrhip_channelizer *h, const double *taps) {
  return guarded([&] {
    SDRHIP_REQUIRE(h && taps, SDRHIP_E_INVALID, "NULL argument");
    h->ctx->use();
    h->set_taps(taps);
  });
}

int sdrhip_channelizer_reset(sdrhip_channelizer *h) {
  return guarded([&] {
    use_handle(h);
    h->fresh_tail();
  });
}

int sdrhip_channelizer_get_state(sdrhip_channelizer *h, uint64_t *consumed, float *tail, size_t tail_len) {
  return guarded([&] {
    use_handle(h);
    h->get_tail(consumed, tail, tail_len);
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
    write_names(h, buf, len, [&] { return CH_NAMES[h->real][h->dtype != SDRHIP_CHAN_CS16]; });
  });
}

int sdrhip_channelizer_destroy(sdrhip_channelizer *h) {
  return guarded([&] { destroy_handle(h); });
}

}  // extern "C"
