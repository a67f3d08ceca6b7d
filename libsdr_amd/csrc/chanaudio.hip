// chanaudio.hip — the audio channelizer (sdrhip_chanaudio.h): the polyphase channelizer with a demodulator per channel in the
// same launch, int16 audio rows out. Phases 1 and 2 are channelizer_body.hpp's, shared with channelizer.hip, so the spectra have
// the plain channelizer's bits; this file's epilogue is
//   3  all lanes: element (row i, time tt) — the spectrum's bin sel[i] of image halo + tt, times the channel's gain, rounded and
//      clamped to complex<int16>, through the channel's demodulator (fm_phi.hpp), stored as row i's int16 at j0 + tt: Tc
//      contiguous outputs per row. An FM output at call index j >= 2 differences against the angle of the image before it —
//      the tile's own, or the halo image a tile behind the call's first computes for time j0 - 1 when a selected row is FM;
//      j = 1 differences against the channel's `last`, j = 0 is q.re.
// `last` is per channel and double-buffered like the tail: the workgroup holding output n_out - 1 (n_out >= 2) writes every FM
// channel's angle there — selected or not, its image has all M bins — and block 0 copies every other entry.
// A handle of sdrhip_chanreal_audio_create (sdrhip_chanreal.h) runs chanaudio_real_s16_kernel / chanaudio_real_f32_kernel: the body's
// real form in front of the same epilogue; the per-channel arrays then have nch = M / 2 + 1 entries.
// A group of handles (sdrhip_changroup.h) runs group_chanaudio_*_kernel: member blockIdx.y's body (ch_body, as alone) on its own
// arguments; the row call is channelizer_body.hpp's cg_process_rows, as the plain channelizer's.
#include "sdrhip_internal.hpp"
#include "sdrhip_chanaudio.h"
#include "sdrhip_chanreal.h"
#include "entry.hpp"
#include "channelizer_body.hpp"
#include "fm_phi.hpp"

#include <algorithm>
#include <cmath>

using namespace sdrhip;

namespace {

struct ChAudioArgs {
  ChArgs c;
  const int *mode;      // [nch] SDRHIP_EPI_FM | _AM | _USB
  const float *gain;    // [nch]
  const int *last;      // [nch] the angles before the call
  int *last_new;        // [nch] behind it
  int fm_rows;          // selected rows that are FM
};

// one float32 multiply, round to nearest even, NaN -> 0, clamp
__device__ __forceinline__ int ca_conv(float g, float v) {
  const float p = g * v;
  const float r = p != p ? 0.f : __builtin_rintf(p);
  return (int)__builtin_fminf(__builtin_fmaxf(r, -32768.f), 32767.f);
}
__device__ __forceinline__ int ca_phi(float g, float2 y) { return fm_phi(ca_conv(g, y.x), ca_conv(g, y.y)); }

struct ChStoreAudio {
  const ChAudioArgs &x;
  __device__ __forceinline__ int halo(const ChArgs &, int j0) const { return j0 >= 1 && x.fm_rows > 0 ? 1 : 0; }
  __device__ __forceinline__ void store(const ChArgs &a, const float2 *img, int j0, int Tc, int halo, int tid) const {
    short *out = static_cast<short *>(a.out);
    for (int e = tid; e < a.n_sel * Tc; e += CH_THREADS) {
      const int i = e / Tc, tt = e - i * Tc, j = j0 + tt, k = a.sel[i], mode = x.mode[k];
      const float g = x.gain[k];
      const float2 *y = img + (halo + tt) * a.ld + k;
      const int re = ca_conv(g, y->x), im = ca_conv(g, y->y);
      short o;
      if (mode == SDRHIP_EPI_AM) o = am_i16(re, im);
      else if (mode == SDRHIP_EPI_USB) o = usb_i16(re, im);
      else if (j == 0) o = (short)re;
      else {
        // (halo + tt >= 1 wherever j >= 2: tt >= 1, or the tile has its halo image because this row is FM — the test keeps a
        // wrong count from becoming a read before the images)
        const int prev = j == 1 || halo + tt == 0 ? x.last[k] : ca_phi(g, y[-a.ld]);
        o = (short)(prev - fm_phi(re, im));
      }
      out[(long)i * a.out_stride + j] = o;
    }
    // the angles behind the call: the last output's, of every FM channel
    if (a.n_out >= 2 && j0 + Tc == a.n_out) {
      const float2 *y = img + (halo + Tc - 1) * a.ld;
      for (int k = tid; k < a.M; k += CH_THREADS)
        if (x.mode[k] == SDRHIP_EPI_FM) x.last_new[k] = ca_phi(x.gain[k], y[k]);
    }
  }
  template <class I>
  __device__ __forceinline__ void roll(const ChArgs &a, int tid) const {
    ch_roll_tail<I>(a, tid);
    if (blockIdx.x == 0)
      for (int k = tid; k < a.M; k += CH_THREADS)
        if (!(a.n_out >= 2 && x.mode[k] == SDRHIP_EPI_FM)) x.last_new[k] = x.last[k];
  }
};

__global__ __launch_bounds__(CH_THREADS) void chanaudio_cs16_kernel(const ChAudioArgs a) { ch_body<short2>(a.c, ChStoreAudio{a}); }
__global__ __launch_bounds__(CH_THREADS) void chanaudio_cf32_kernel(const ChAudioArgs a) { ch_body<float2>(a.c, ChStoreAudio{a}); }
__global__ __launch_bounds__(CH_THREADS) void chanaudio_real_s16_kernel(const ChAudioArgs a) { ch_body<short>(a.c, ChStoreAudio{a}); }
__global__ __launch_bounds__(CH_THREADS) void chanaudio_real_f32_kernel(const ChAudioArgs a) { ch_body<float>(a.c, ChStoreAudio{a}); }

// a group launch (sdrhip_changroup.h): member blockIdx.y's body on its own arguments
using CaGroupArgs = ChGroupArgs<ChAudioArgs>;
static_assert(sizeof(CaGroupArgs) <= CG_ARG_BYTES, "the member table travels in the kernel arguments");
__global__ __launch_bounds__(CH_THREADS) void group_chanaudio_cs16_kernel(const CaGroupArgs g) {
  const ChAudioArgs &a = g.m[blockIdx.y];
  ch_body<short2>(a.c, ChStoreAudio{a});
}
__global__ __launch_bounds__(CH_THREADS) void group_chanaudio_cf32_kernel(const CaGroupArgs g) {
  const ChAudioArgs &a = g.m[blockIdx.y];
  ch_body<float2>(a.c, ChStoreAudio{a});
}
__global__ __launch_bounds__(CH_THREADS) void group_chanaudio_real_s16_kernel(const CaGroupArgs g) {
  const ChAudioArgs &a = g.m[blockIdx.y];
  ch_body<short>(a.c, ChStoreAudio{a});
}
__global__ __launch_bounds__(CH_THREADS) void group_chanaudio_real_f32_kernel(const CaGroupArgs g) {
  const ChAudioArgs &a = g.m[blockIdx.y];
  ch_body<float>(a.c, ChStoreAudio{a});
}

using CaKernel = void (*)(const ChAudioArgs);
using CaGroupKernel = void (*)(const CaGroupArgs);
constexpr CaGroupKernel CAG_KERNELS[2][2] = {{group_chanaudio_cs16_kernel, group_chanaudio_cf32_kernel},
                                             {group_chanaudio_real_s16_kernel, group_chanaudio_real_f32_kernel}};
constexpr const char *CAG_NAMES[2][2] = {{"group_chanaudio_cs16_kernel", "group_chanaudio_cf32_kernel"},
                                         {"group_chanaudio_real_s16_kernel", "group_chanaudio_real_f32_kernel"}};
constexpr CaKernel CA_KERNELS[2][2] = {{chanaudio_cs16_kernel, chanaudio_cf32_kernel}, {chanaudio_real_s16_kernel, chanaudio_real_f32_kernel}};
constexpr const char *CA_NAMES[2][2] = {{"chanaudio_cs16_kernel", "chanaudio_cf32_kernel"}, {"chanaudio_real_s16_kernel", "chanaudio_real_f32_kernel"}};

// SDRHIP_EPI_NONE has a code of its own: its rows would have another element size
void require_mode(int mode, const char *what, int index) {
  SDRHIP_REQUIRE(mode != SDRHIP_EPI_NONE, SDRHIP_E_UNSUPPORTED, "mode of %s %d is SDRHIP_EPI_NONE: the node makes audio rows, not complex<int16> ones",
                 what, index);
  SDRHIP_REQUIRE(mode == SDRHIP_EPI_FM || mode == SDRHIP_EPI_AM || mode == SDRHIP_EPI_USB, SDRHIP_E_INVALID,
                 "mode %d of %s %d is none of SDRHIP_EPI_FM, _AM, _USB", mode, what, index);
}
void require_gain(float gain, const char *what, int index) {
  SDRHIP_REQUIRE(std::isfinite(gain), SDRHIP_E_INVALID, "gain of %s %d is not finite", what, index);
}

}  // namespace

struct sdrhip_chanaudio : ChPlan {
  std::vector<int> mode_host;      // [nch]
  std::vector<float> gain_host;    // [nch]
  DevBuf<int> mode, last[2];       // [nch] each; last[cur] holds the state (the buffers flip with the tail's)
  DevBuf<float> gain;              // [nch]
  CaKernel kernel() const { return pick(CA_KERNELS); }
  size_t lds_bytes() const { return (size_t)(T + 1) * (size_t)ld * sizeof(float2); }
  int fm_rows() const {
    int n = 0;
    for (int k : sel_host) n += mode_host[(size_t)k] == SDRHIP_EPI_FM;
    return n;
  }
  void fresh_state() {
    SDRHIP_CHECK_HIP(hipMemsetAsync(last[0].p, 0, (size_t)nch * sizeof(int), ctx->stream));
    fresh_tail();   // (synchronises, and cur = 0)
  }
  void require_row(int row) const { SDRHIP_REQUIRE(row >= 0 && row < n_sel, SDRHIP_E_INVALID, "row %d outside [0,%d)", row, n_sel); }
  // the arguments of a launch of n >= 1 samples from the current state
  ChAudioArgs audio_args(const void *in_dev, size_t n, void *out_dev, size_t out_stride, size_t n_out) const {
    ChAudioArgs a;
    a.c = args(in_dev, n, out_dev, out_stride, n_out);
    a.mode = mode.p; a.gain = gain.p; a.last = last[cur].p; a.last_new = last[cur ^ 1].p;
    a.fm_rows = fm_rows();
    return a;
  }
  // n >= 1
  void launch(const void *in_dev, size_t n, void *out_dev, size_t out_stride, size_t n_out) {
    ctx->use();
    const ChAudioArgs a = audio_args(in_dev, n, out_dev, out_stride, n_out);
    launch_tiles(kernel(), a.c.tiles, lds_bytes(), n, a);
  }
};

namespace {

// both create calls; real: sdrhip_chanreal.h's, K = M / 2 + 1 channels (the rules before have made M even)
int create(sdrhip_ctx *ctx, int dtype, int M, int D, const double *taps, int n_taps, size_t max_in, const int *modes, const float *gains,
           sdrhip_chanaudio **out, bool real) {
  int K = 0;
  return ch_create(
      ctx, dtype, M, D, taps, n_taps, max_in, out, real,
      [&] {
        K = real ? M / 2 + 1 : M;
        for (int k = 0; modes && k < K; k++) require_mode(modes[k], "channel", k);
        for (int k = 0; gains && k < K; k++) require_gain(gains[k], "channel", k);
      },
      [&](sdrhip_chanaudio *h) {
        h->mode_host.assign((size_t)K, SDRHIP_EPI_FM);
        h->gain_host.assign((size_t)K, 1.0f);
        if (modes) h->mode_host.assign(modes, modes + K);
        if (gains) h->gain_host.assign(gains, gains + K);
        h->mode.alloc((size_t)K);
        h->mode.upload(h->mode_host.data(), (size_t)K, ctx->stream);
        h->gain.alloc((size_t)K);
        h->gain.upload(h->gain_host.data(), (size_t)K, ctx->stream);
        for (auto &b : h->last) { b.alloc((size_t)K); b.zero(ctx->stream); }
      });
}

// get_modes / get_gains: row i's entry of the per-channel host array; short_fmt: the message for an array below n_sel entries
template <class X>
int get_rows(sdrhip_chanaudio *h, const std::vector<X> sdrhip_chanaudio::*per_channel, X *rows, int n, const char *short_fmt) {
  return guarded([&] {
    SDRHIP_REQUIRE(h && rows, SDRHIP_E_INVALID, "NULL argument");
    SDRHIP_REQUIRE(n >= h->n_sel, SDRHIP_E_INVALID, short_fmt, n, h->n_sel);
    for (int i = 0; i < h->n_sel; i++) rows[i] = (h->*per_channel)[(size_t)h->sel_host[(size_t)i]];
  });
}

// the row call of an audio group
void group_rows(sdrhip_changroup *g, const void *const *in_dev, const size_t *n, void *const *out_dev, const size_t *out_stride,
                size_t *n_out) {
  cg_process_rows<sdrhip_chanaudio>(g, CAG_KERNELS, sizeof(short), in_dev, n, out_dev, out_stride, n_out,
                                    [](sdrhip_chanaudio *h, const void *in, void *out, const CgCall &c) {
                                      return h->audio_args(in, c.n, out, c.stride, c.no);
                                    });
}

}  // namespace

extern "C" {

int sdrhip_changroup_audio_create(sdrhip_chanaudio *const *members, int count, sdrhip_changroup **out) {
  return cg_create(members, count, out, [](sdrhip_changroup *g) {
    allow_lds_max(g->member[0]->pick(CAG_KERNELS), g->lds);
    g->grid_x = cg_grid_tiles(g);
    g->names = g->member[0]->pick(CAG_NAMES);
    g->rows = group_rows;
  });
}

int sdrhip_chanaudio_create(sdrhip_ctx *ctx, int dtype, int M, int D, const double *taps, int n_taps, size_t max_in, const int *modes,
                            const float *gains, sdrhip_chanaudio **out) {
  return create(ctx, dtype, M, D, taps, n_taps, max_in, modes, gains, out, false);
}

int sdrhip_chanreal_audio_create(sdrhip_ctx *ctx, int dtype, int M, int D, const double *taps, int n_taps, size_t max_in,
                                 const int *modes, const float *gains, sdrhip_chanaudio **out) {
  return create(ctx, dtype, M, D, taps, n_taps, max_in, modes, gains, out, true);
}

int sdrhip_chanaudio_out_count(sdrhip_chanaudio *h, size_t n, size_t *n_out) { return ch_out_count(h, n, n_out); }

int sdrhip_chanaudio_process_dev(sdrhip_chanaudio *h, const void *in_dev, size_t n, void *out_dev, size_t out_stride, size_t *n_out) {
  return ch_process_dev(h, "sdrhip_chanaudio_process_dev", sizeof(short), in_dev, n, out_dev, out_stride, n_out);
}

int sdrhip_chanaudio_process(sdrhip_chanaudio *h, const void *in_host, size_t n, void *out_host, size_t out_stride, size_t *n_out) {
  return ch_process(h, "sdrhip_chanaudio_process", sizeof(short), in_host, n, out_host, out_stride, n_out);
}

int sdrhip_chanaudio_set_channels(sdrhip_chanaudio *h, const int *idx, int n_sel) { return ch_set_channels(h, idx, n_sel); }

int sdrhip_chanaudio_set_mode(sdrhip_chanaudio *h, int row, int mode) {
  return guarded([&] {
    SDRHIP_REQUIRE(h, SDRHIP_E_INVALID, "handle is NULL");
    h->require_row(row);
    require_mode(mode, "row", row);
    h->ctx->use();
    // stream-ordered after the launches already enqueued: the mode, and behind it the row's `last` = 0
    const size_t k = (size_t)h->sel_host[(size_t)row];
    const int zero = 0;
    replace_row(h->ctx, h->mode.p + k, h->mode_host[k], mode, h->last[h->cur].p + k, &zero, sizeof zero);
  });
}

int sdrhip_chanaudio_get_modes(sdrhip_chanaudio *h, int *modes, int n) {
  return get_rows(h, &sdrhip_chanaudio::mode_host, modes, n, "modes holds %d entries, the node writes %d rows");
}

int sdrhip_chanaudio_set_gain(sdrhip_chanaudio *h, int row, float gain) {
  return guarded([&] {
    SDRHIP_REQUIRE(h, SDRHIP_E_INVALID, "handle is NULL");
    h->require_row(row);
    require_gain(gain, "row", row);
    h->ctx->use();
    const int k = h->sel_host[(size_t)row];
    put_sync(h->ctx, h->gain.p + k, &gain, sizeof(float));
    h->gain_host[(size_t)k] = gain;
  });
}

int sdrhip_chanaudio_get_gains(sdrhip_chanaudio *h, float *gains, int n) {
  return get_rows(h, &sdrhip_chanaudio::gain_host, gains, n, "gains holds %d entries, the node writes %d rows");
}

int sdrhip_chanaudio_set_taps(sdrhip_chanaudio *h, const double *taps) { return ch_set_taps(h, taps); }

int sdrhip_chanaudio_reset(sdrhip_chanaudio *h) { return ch_reset(h); }

int sdrhip_chanaudio_get_state(sdrhip_chanaudio *h, uint64_t *consumed, float *tail, size_t tail_len, int *last, size_t n_last) {
  return guarded([&] {
    use_handle(h);
    SDRHIP_REQUIRE(!last || n_last >= (size_t)h->n_sel, SDRHIP_E_SIZE, "n_last %zu < rows = %d", n_last, h->n_sel);
    h->get_tail(consumed, tail, tail_len);
    if (last) {
      std::vector<int> all((size_t)h->nch);
      get_sync(h->ctx, all.data(), h->last[h->cur].p, all.size() * sizeof(int));
      for (int i = 0; i < h->n_sel; i++) last[i] = all[(size_t)h->sel_host[(size_t)i]];
    }
  });
}

int sdrhip_chanaudio_plan_info(sdrhip_chanaudio *h, int *tile_times, int *branch_taps, int *lds_bytes, int *rows, int *fm_rows,
                               int *halo_tiles) {
  return guarded([&] {
    ch_plan_head(h, tile_times, branch_taps, lds_bytes);
    if (rows) *rows = h->n_sel;
    if (fm_rows) *fm_rows = h->fm_rows();
    if (halo_tiles) {
      const size_t tiles = ceil_div(h->out_count(h->max_in), (size_t)h->T);
      *halo_tiles = h->fm_rows() > 0 && tiles > 0 ? (int)(tiles - 1) : 0;
    }
  });
}

int sdrhip_chanaudio_kernel_names(sdrhip_chanaudio *h, char *buf, size_t len) { return ch_kernel_names(h, buf, len, CA_NAMES); }

int sdrhip_chanaudio_destroy(sdrhip_chanaudio *h) {
  return guarded([&] { destroy_handle(h); });
}

}  // extern "C"
