// rxbank.hip — the receiver bank (sdrhip_rx.h): tuner bank -> FMDeemph -> detector -> bit stream of every channel of ONE
// antenna, enqueued by one call on the context's stream with nothing leaving the device in between. Host code only: the
// kernels are the components', reached through their public *_process_dev entry points, so a receiver bank computes what
// the same handles chained by hand compute. What it adds is the rows between the stages and every size between them.
#include "sdrhip_internal.hpp"
#include "sdrhip_rx.h"
#include "entry.hpp"

using namespace sdrhip;

// a component's entry point inside guarded(): its code and its sdrhip_last_error text become this call's
#define RX_CALL(expr)                          \
  do {                                         \
    const int c_ = (expr);                     \
    if (c_ != SDRHIP_OK) throw Failure{c_};    \
  } while (0)

struct sdrhip_rxbank {
  sdrhip_ctx *ctx = nullptr;
  sdrhip_tuner_i16 *tuner = nullptr;   // borrowed, all four
  sdrhip_deemph *deemph = nullptr;
  sdrhip_detector *det = nullptr;
  sdrhip_bits *bits = nullptr;
  int C = 1;
  size_t max_in = 0, max_audio = 0, stride = 0;   // stride: the owned rows', max_audio rounded up to whole 16 bytes
  DevBuf<short> demod, audio;   // the tuner's rows; the de-emphasised ones (allocated only with a de-emphasis stage)
  DevBuf<uint8_t> sym;
  // the host-pointer call's device side, allocated by the first one
  DevBuf<uint8_t> st_in, st_bits;
  DevBuf<uint32_t> st_counts;
  DevBuf<short> st_audio;

  size_t n_audio(size_t n_in) const {
    size_t na = 0;
    RX_CALL(sdrhip_tuner_i16_out_count(tuner, n_in, &na));
    return na;
  }
  size_t capacity(size_t na) const {
    size_t cap = 0;
    RX_CALL(sdrhip_bits_out_capacity(bits, na, &cap));
    return cap;
  }

  // every argument rule first: a call that fails leaves no stage ahead of the others
  void run(const void *in_dev, size_t n_in, uint8_t *bits_dev, size_t bits_stride, uint32_t *counts_dev, short *audio_dev,
           size_t audio_stride, size_t *n_audio_out) {
    SDRHIP_REQUIRE(counts_dev, SDRHIP_E_INVALID, "NULL argument");
    SDRHIP_REQUIRE(n_in <= max_in, SDRHIP_E_SIZE, "n_in %zu > max_in %zu", n_in, max_in);
    const size_t na = n_in ? n_audio(n_in) : 0;
    if (n_audio_out) *n_audio_out = na;
    SDRHIP_REQUIRE(na <= max_audio, SDRHIP_E_SIZE, "%zu samples per audio row > %zu", na, max_audio);
    size_t a_stride = stride;
    if (na) {
      SDRHIP_REQUIRE(in_dev && bits_dev, SDRHIP_E_INVALID, "NULL buffer");
      const size_t cap = capacity(na);
      if (bits_stride == 0) bits_stride = cap;
      SDRHIP_REQUIRE(bits_stride >= cap, SDRHIP_E_SIZE, "bits_stride %zu < capacity %zu", bits_stride, cap);
      if (audio_dev) {
        a_stride = audio_stride ? audio_stride : na;
        SDRHIP_REQUIRE(a_stride >= na, SDRHIP_E_SIZE, "audio_stride %zu < n_audio %zu", a_stride, na);
      }
    } else if (n_in) SDRHIP_REQUIRE(in_dev, SDRHIP_E_INVALID, "NULL buffer");
    if (n_in) {
      // the rows the detector reads are the caller's audio rows where it asked for them, the bank's own where not
      short *last = audio_dev && na ? audio_dev : (deemph ? audio.p : demod.p);
      short *first = deemph ? demod.p : last;
      size_t got = 0;
      RX_CALL(sdrhip_tuner_i16_process_dev(tuner, in_dev, n_in, first, deemph ? stride : a_stride, &got));
      SDRHIP_REQUIRE(got == na, SDRHIP_E_INVALID, "the tuner produced %zu samples per row, not %zu", got, na);
      if (na) {
        if (deemph) RX_CALL(sdrhip_deemph_i16_process_dev(deemph, first, na, stride, last, a_stride));
        RX_CALL(sdrhip_detector_process_dev(det, last, na, a_stride, sym.p, stride));
        RX_CALL(sdrhip_bits_process_dev(bits, sym.p, na, stride, bits_dev, bits_stride, counts_dev));
        return;
      }
    }
    RX_CALL(sdrhip_bits_process_dev(bits, nullptr, 0, 0, nullptr, 0, counts_dev));   // no symbol: every count 0, nothing else moves
  }
};

extern "C" {

int sdrhip_rxbank_create(sdrhip_ctx *ctx, sdrhip_tuner_i16 *tuner, sdrhip_deemph *deemph, sdrhip_detector *detector,
                         sdrhip_bits *bits, sdrhip_rxbank **out) {
  return guarded([&] {
    if (out) *out = nullptr;
    SDRHIP_REQUIRE(tuner && detector && bits && out, SDRHIP_E_INVALID, "NULL argument");
    require_device_for_null_ctx(ctx);
    make_handle(ctx, out, true, [&](sdrhip_rxbank *h) {
      SDRHIP_REQUIRE(handle_ctx(tuner) == ctx && (!deemph || handle_ctx(deemph) == ctx) && handle_ctx(detector) == ctx &&
                         handle_ctx(bits) == ctx,
                     SDRHIP_E_INVALID, "a component belongs to another context");
      SDRHIP_REQUIRE(tuner_epilogue(tuner) != SDRHIP_EPI_NONE, SDRHIP_E_UNSUPPORTED,
                     "the tuner's rows are cs16 (SDRHIP_EPI_NONE): a receiver needs a demodulator behind every channel");
      const int C = handle_channels(tuner);
      SDRHIP_REQUIRE((!deemph || handle_channels(deemph) == C) && handle_channels(detector) == C && handle_channels(bits) == C,
                     SDRHIP_E_INVALID, "channels differ: tuner %d, de-emphasis %d, detector %d, bits %d", C,
                     deemph ? handle_channels(deemph) : C, handle_channels(detector), handle_channels(bits));
      const size_t max_audio = ceil_div(handle_max_in(tuner), (size_t)tuner_decim(tuner));
      SDRHIP_REQUIRE((!deemph || handle_max_in(deemph) >= max_audio) && handle_max_in(detector) >= max_audio &&
                         handle_max_in(bits) >= max_audio,
                     SDRHIP_E_SIZE, "a later stage's max_in (de-emphasis %zu, detector %zu, bits %zu) < %zu = ceil(tuner max_in / decimation)",
                     deemph ? handle_max_in(deemph) : max_audio, handle_max_in(detector), handle_max_in(bits), max_audio);
      h->tuner = tuner; h->deemph = deemph; h->det = detector; h->bits = bits;
      h->C = C; h->max_in = handle_max_in(tuner); h->max_audio = max_audio; h->stride = (max_audio + 7) & ~(size_t)7;
      h->demod.alloc((size_t)C * h->stride);
      if (deemph) h->audio.alloc((size_t)C * h->stride);
      h->sym.alloc((size_t)C * h->stride);
    });
  });
}

int sdrhip_rxbank_sizes(sdrhip_rxbank *h, size_t n_in, size_t *n_audio, size_t *bits_cap) {
  return guarded([&] {
    SDRHIP_REQUIRE(h, SDRHIP_E_INVALID, "handle is NULL");
    const size_t na = n_in ? h->n_audio(n_in) : 0;
    if (n_audio) *n_audio = na;
    if (bits_cap) *bits_cap = h->capacity(na);
  });
}

int sdrhip_rxbank_process_dev(sdrhip_rxbank *h, const void *in_dev, size_t n_in, uint8_t *bits_dev, size_t bits_stride,
                              uint32_t *counts_dev, int16_t *audio_dev, size_t audio_stride, size_t *n_audio) {
  return guarded([&] {
    Range roctx_range("sdrhip_rxbank_process_dev");
    SDRHIP_REQUIRE(h, SDRHIP_E_INVALID, "handle is NULL");
    h->ctx->use();
    h->run(in_dev, n_in, bits_dev, bits_stride, counts_dev, audio_dev, audio_stride, n_audio);
  });
}

int sdrhip_rxbank_process(sdrhip_rxbank *h, const void *in_host, size_t n_in, uint8_t *bits_host, size_t bits_stride,
                          uint32_t *counts_host, int16_t *audio_host, size_t audio_stride, size_t *n_audio) {
  return guarded([&] {
    Range roctx_range("sdrhip_rxbank_process");
    SDRHIP_REQUIRE(h && counts_host, SDRHIP_E_INVALID, "NULL argument");
    SDRHIP_REQUIRE(n_in <= h->max_in, SDRHIP_E_SIZE, "n_in %zu > max_in %zu", n_in, h->max_in);
    SDRHIP_REQUIRE(!n_in || in_host, SDRHIP_E_INVALID, "NULL buffer");
    sdrhip_ctx *ctx = h->ctx;
    ctx->use();
    const size_t C = (size_t)h->C, na = n_in ? h->n_audio(n_in) : 0, cap = h->capacity(na);
    if (na) {
      SDRHIP_REQUIRE(bits_host, SDRHIP_E_INVALID, "NULL buffer");
      if (bits_stride == 0) bits_stride = cap;
      SDRHIP_REQUIRE(bits_stride >= cap, SDRHIP_E_SIZE, "bits_stride %zu < capacity %zu", bits_stride, cap);
      if (audio_host && audio_stride == 0) audio_stride = na;
      SDRHIP_REQUIRE(!audio_host || audio_stride >= na, SDRHIP_E_SIZE, "audio_stride %zu < n_audio %zu", audio_stride, na);
    }
    const size_t ib = tuner_in_elem_bytes(h->tuner);
    if (!h->st_in.p) { h->st_in.alloc(h->max_in * 4); h->st_counts.alloc(C); h->st_audio.alloc(C * h->stride); }
    // (a set_channel to a faster baud rate raises the capacity the staged rows need)
    if (h->st_bits.n < C * std::max(cap, h->capacity(h->max_audio))) h->st_bits.alloc(C * std::max(cap, h->capacity(h->max_audio)));
    if (n_in) copy_h2d_rows(ctx, h->st_in.p, n_in * ib, in_host, n_in * ib, n_in * ib, 1);
    h->st_bits.zero(ctx->stream);   // the bytes of a row behind counts[c] reach the caller as zeros
    h->run(h->st_in.p, n_in, h->st_bits.p, cap, h->st_counts.p, audio_host ? h->st_audio.p : nullptr, h->stride, n_audio);
    SDRHIP_CHECK_HIP(hipMemcpyAsync(counts_host, h->st_counts.p, C * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (na) {
      copy_d2h_rows(ctx, bits_host, bits_stride, h->st_bits.p, cap, cap, C);
      if (audio_host) copy_d2h_rows(ctx, audio_host, audio_stride * 2, h->st_audio.p, h->stride * 2, na * 2, C);
    }
    SDRHIP_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  });
}

int sdrhip_rxbank_destroy(sdrhip_rxbank *h) {
  return guarded([&] { destroy_handle(h); });
}

}  // extern "C"
