// baudot.hip — the Baudot decoder bank (sdrhip_baudot.h): `channels` reference Baudot nodes (src/baudot.cc:86-111), one wave of
// 64 lanes per row, BD_WAVES rows per workgroup, one launch per call. The reference's per-bit loop is restated for 64
// positions at a time:
//   1. a ballot packs the chunk's half-bits into one word; with the word before it every lane has the 16 bits _bitstream
//      holds at its position and tests them against the row's mask and pattern: the candidate mask;
//   2. the gate "bitsPerSymbol <= _bitcount" is a greedy pick over that mask — the first candidate at or behind
//      next_allowed is taken, next_allowed moves bitsPerSymbol behind it — in wave-uniform scalar code, five trips at most;
//   3. a taken lane's table is set by the highest shift code below it in the chunk, or is the carried one;
//   4. the emitting lanes compact by the population count of the emit mask below them.
// Nothing in it walks a row bit by bit, and no lane indexes a private array: the two tables live in constant memory.
#include "sdrhip_internal.hpp"
#include "sdrhip_baudot.h"
#include "entry.hpp"

using namespace sdrhip;

namespace {

constexpr int BD_CHANNELS_MAX = 8192;
constexpr size_t BD_BITS_MAX = 65536;
constexpr int BD_WAVES = 4;   // rows per workgroup
constexpr unsigned BD_STL = 31, BD_STF = 27, BD_SPA = 4;   // shift to letters, shift to figures, space

// The two code tables (sdrhip_baudot.h): ITA2 with the code's bit 0 as the lowest data bit. BEL is figures 5; both line
// codes (2 and 8) give '\n'; the places of the null and of the two shift codes hold 0.
__constant__ unsigned char BD_LETTERS[32] = {0,   'E', '\n', 'A', ' ', 'S', 'I', 'U', '\n', 'D', 'R', 'J', 'N', 'F', 'C', 'K',
                                             'T', 'Z', 'L',  'W', 'H', 'Y', 'P', 'Q', 'O',  'B', 'G', 0,   'M', 'X', 'V', 0};
__constant__ unsigned char BD_FIGURES[32] = {0,   '3', '\n', '-', ' ', '\a', '8', '7', '\n', '?', '4', '\'', ',', '!', ':', '(',
                                             '5', '"', ')',  '2', '#', '6',  '0', '1', '9',  '?', '&', 0,    '.', '/', ';', 0};

// the reference node's protected members, one set per row
struct BdRegs {
  unsigned long long bitcount;   // _bitcount
  unsigned bitstream, pad_;      // _bitstream (16 bits)
};

struct BdArgs {
  const uint8_t *bits; long bits_stride; const unsigned *counts;
  uint8_t *text; long text_stride; unsigned *out_counts; unsigned *status;
  BdRegs *regs; unsigned *mode; const int *stops; const int *enabled;
  unsigned max_bits, channels;
};

// _bitstream after the half-bit at chunk position l: positions l ... l-15, the newest in bit 0. `cur` holds the chunk's
// positions 0 ... 63 in bits 0 ... 63, `prev` the 64 positions before them.
__device__ inline unsigned bd_window(unsigned long long prev, unsigned long long cur, unsigned l) {
  const unsigned s = 49 + l;   // the window's oldest bit, counted from prev's bit 0
  const unsigned long long x = s < 64 ? (prev >> s) | (cur << (64 - s)) : cur >> (s - 64);
  return __brev((unsigned)x & 0xFFFFu) >> 16;
}

__global__ __launch_bounds__(64 * BD_WAVES) void baudot_decode_kernel(BdArgs a) {
  const unsigned lane = threadIdx.x & 63;
  const unsigned c = blockIdx.x * BD_WAVES + (threadIdx.x >> 6);
  if (c >= a.channels) return;   // (whole waves: a row is a wave's, and nothing below synchronises the workgroup)
  if (!a.enabled[c]) {
    if (lane == 0) a.out_counts[c] = 0;
    return;
  }
  unsigned n = a.counts[c];
  if (n > a.max_bits) {
    n = a.max_bits;
    if (lane == 0) *a.status = 1;
  }
  const unsigned stop_h = 2u + (unsigned)a.stops[c], bps = 12u + stop_h;
  const unsigned mask = (3u << (bps - 2)) | ((1u << stop_h) - 1u), pattern = 3u << (bps - 2);
  const BdRegs s = a.regs[c];
  unsigned mode = a.mode[c];
  const uint8_t *row = a.bits + (long)c * a.bits_stride;
  uint8_t *text = a.text + (long)c * a.text_stride;

  // carried _bitstream: its bit 0 is position -1, so the bit-reversed word has it in bit 63
  unsigned long long prev = __brevll((unsigned long long)(s.bitstream & 0xFFFFu)), cur = 0;
  // the first position of this call at which the gate lets a symbol through: carried + i + 1 >= bps
  unsigned next_allowed = s.bitcount >= bps - 1 ? 0u : bps - 1 - (unsigned)s.bitcount;
  unsigned nout = 0, last = 0;
  bool any = false;
  const unsigned long long below = (1ull << lane) - 1;
  const unsigned chunks = (n + 63) >> 6;
  for (unsigned k = 0; k < chunks; k++) {
    const unsigned base = k * 64, p = base + lane;
    const bool valid = p < n;
    const int bit = valid ? (row[p] & 1) : 0;
    if (k) prev = cur;
    cur = __ballot(bit);
    const unsigned w = bd_window(prev, cur, lane);
    unsigned long long cand = __ballot(valid && (w & mask) == pattern);
    // the gate, wave-uniform: at most ceil(64 / 14) = 5 symbols in a chunk
    unsigned long long taken = 0;
    while (cand) {
      const unsigned lo = next_allowed > base ? next_allowed - base : 0;
      if (lo >= 64) break;
      cand &= ~0ull << lo;
      if (!cand) break;
      const unsigned f = (unsigned)__ffsll((long long)cand) - 1;
      taken |= 1ull << f;
      last = base + f;
      any = true;
      next_allowed = last + bps;
    }
    if (!taken) continue;
    const bool mine = (taken >> lane) & 1;
    unsigned code = 0;
#pragma unroll
    for (unsigned j = 0; j < 5; j++) code |= ((w >> (stop_h + 2 * j)) & 1u) << j;
    const unsigned long long to_l = __ballot(mine && (code == BD_STL || code == BD_SPA));
    const unsigned long long to_f = __ballot(mine && code == BD_STF);
    const unsigned long long emit = __ballot(mine && code != BD_STL && code != BD_STF);
    // the setters are disjoint, so the greater of the two masks below a lane holds the highest setter below it
    const unsigned long long bl = to_l & below, bf = to_f & below;
    const unsigned my_mode = code == BD_SPA ? (unsigned)SDRHIP_BAUDOT_LETTERS : (bl | bf) ? (unsigned)(bf > bl) : mode;
    if ((emit >> lane) & 1) {
      const unsigned at = nout + (unsigned)__popcll(emit & below);
      if ((long)at < a.text_stride) text[at] = my_mode == SDRHIP_BAUDOT_FIGURES ? BD_FIGURES[code] : BD_LETTERS[code];
    }
    nout += (unsigned)__popcll(emit);
    if (to_l | to_f) mode = to_f > to_l;
  }
  if (lane == 0) {
    if (n) {
      BdRegs o;
      o.bitstream = bd_window(prev, cur, (n - 1) & 63);
      o.bitcount = any ? (unsigned long long)(n - 1 - last) : s.bitcount + n;
      o.pad_ = 0;
      a.regs[c] = o;
      a.mode[c] = mode;
    }
    a.out_counts[c] = (long)nout < a.text_stride ? nout : (unsigned)a.text_stride;
  }
}

bool bd_stop_ok(int stop) { return stop == SDRHIP_BAUDOT_STOP1 || stop == SDRHIP_BAUDOT_STOP15 || stop == SDRHIP_BAUDOT_STOP2; }

}  // namespace

struct sdrhip_baudot {
  sdrhip_ctx *ctx = nullptr;
  int C = 1;
  size_t max_bits = 0, cap = 0;   // cap: sdrhip_baudot_out_capacity(max_bits), the smallest text-row stride
  std::vector<int> stops, enabled;
  DevBuf<int> stops_dev, en_dev;
  DevBuf<BdRegs> regs;
  DevBuf<unsigned> mode, status;
  // the host-pointer call's two sides, grown by the calls that need them
  std::vector<uint8_t> host_bits;
  DevBuf<uint8_t> st_bits, st_text;
  DevBuf<unsigned> st_counts, st_outc;

  void launch(const uint8_t *bits_dev, size_t bits_stride, const unsigned *counts_dev, uint8_t *text_dev, size_t text_stride,
              unsigned *out_counts_dev, unsigned *status_dev) {
    SDRHIP_REQUIRE(bits_dev && counts_dev && text_dev && out_counts_dev, SDRHIP_E_INVALID, "NULL buffer");
    if (bits_stride == 0) bits_stride = max_bits;
    if (text_stride == 0) text_stride = cap;
    SDRHIP_REQUIRE(text_stride >= cap, SDRHIP_E_SIZE, "text_stride %zu < capacity %zu of max_bits %zu", text_stride, cap, max_bits);
    if (!status_dev) status_dev = status.p;
    SDRHIP_CHECK_HIP(hipMemsetAsync(status_dev, 0, sizeof(unsigned), ctx->stream));
    BdArgs a;
    a.bits = bits_dev; a.bits_stride = (long)bits_stride; a.counts = counts_dev;
    a.text = text_dev; a.text_stride = (long)text_stride; a.out_counts = out_counts_dev; a.status = status_dev;
    a.regs = regs.p; a.mode = mode.p; a.stops = stops_dev.p; a.enabled = en_dev.p;
    a.max_bits = (unsigned)max_bits; a.channels = (unsigned)C;
    hipLaunchKernelGGL(baudot_decode_kernel, dim3((unsigned)ceil_div((size_t)C, (size_t)BD_WAVES)), dim3(64 * BD_WAVES), 0, ctx->stream, a);
    SDRHIP_CHECK_HIP(hipGetLastError());
  }
  void reset_rows(int first, int rows, int keep_mode) {
    SDRHIP_CHECK_HIP(hipMemsetAsync(regs.p + first, 0, (size_t)rows * sizeof(BdRegs), ctx->stream));
    if (!keep_mode) SDRHIP_CHECK_HIP(hipMemsetAsync(mode.p + first, 0, (size_t)rows * sizeof(unsigned), ctx->stream));
  }
};

namespace {

// both create calls behind their own argument rules
void bd_create(sdrhip_ctx *ctx, const int *stops, int one_stop, const int *enabled, int channels, size_t max_bits, sdrhip_baudot **out) {
  require_device_for_null_ctx(ctx);
  make_handle(ctx, out, true, [&](sdrhip_baudot *h) {
    h->C = channels; h->max_bits = max_bits; h->cap = sdrhip_baudot_out_capacity(max_bits);
    h->stops.resize((size_t)channels);
    h->enabled.resize((size_t)channels);
    for (int c = 0; c < channels; c++) {
      h->stops[c] = stops ? stops[c] : one_stop;
      h->enabled[c] = enabled ? enabled[c] != 0 : 1;
    }
    h->stops_dev.alloc((size_t)channels);
    h->stops_dev.upload(h->stops.data(), h->stops.size(), ctx->stream);
    h->en_dev.alloc((size_t)channels);
    h->en_dev.upload(h->enabled.data(), h->enabled.size(), ctx->stream);
    h->regs.alloc((size_t)channels);
    h->regs.zero(ctx->stream);
    h->mode.alloc((size_t)channels);
    h->mode.zero(ctx->stream);
    h->status.alloc(1);
    h->status.zero(ctx->stream);
  });
}

void bd_require_max_bits(size_t max_bits) {
  SDRHIP_REQUIRE(max_bits >= 1 && max_bits <= BD_BITS_MAX, SDRHIP_E_SIZE, "max_bits %zu outside [1,%zu]", max_bits, BD_BITS_MAX);
}

}  // namespace

extern "C" {

size_t sdrhip_baudot_out_capacity(size_t n_bits) { return n_bits / 14 + 1; }

int sdrhip_baudot_create(sdrhip_ctx *ctx, int stop, int channels, size_t max_bits, sdrhip_baudot **out) {
  return guarded([&] {
    if (out) *out = nullptr;
    SDRHIP_REQUIRE(out, SDRHIP_E_INVALID, "NULL argument");
    SDRHIP_REQUIRE(bd_stop_ok(stop), SDRHIP_E_INVALID, "stop %d is none of STOP1, STOP15, STOP2", stop);
    require_channels(channels, BD_CHANNELS_MAX);
    bd_require_max_bits(max_bits);
    bd_create(ctx, nullptr, stop, nullptr, channels, max_bits, out);
  });
}

int sdrhip_baudotbank_create(sdrhip_ctx *ctx, const int *stops, const int *enabled, int channels, size_t max_bits, sdrhip_baudot **out) {
  return guarded([&] {
    if (out) *out = nullptr;
    SDRHIP_REQUIRE(stops && out, SDRHIP_E_INVALID, "NULL argument");
    require_channels(channels, BD_CHANNELS_MAX);
    bd_require_max_bits(max_bits);
    for (int c = 0; c < channels; c++)
      SDRHIP_REQUIRE(bd_stop_ok(stops[c]), SDRHIP_E_INVALID, "stops[%d] = %d is none of STOP1, STOP15, STOP2", c, stops[c]);
    bd_create(ctx, stops, 0, enabled, channels, max_bits, out);
  });
}

int sdrhip_baudot_process_dev(sdrhip_baudot *h, const uint8_t *bits_dev, size_t bits_stride, const uint32_t *counts_dev,
                              uint8_t *text_dev, size_t text_stride, uint32_t *out_counts_dev, uint32_t *status_dev) {
  return guarded([&] {
    Range roctx_range("sdrhip_baudot_process_dev");
    use_handle(h);
    h->launch(bits_dev, bits_stride, counts_dev, text_dev, text_stride, out_counts_dev, status_dev);
  });
}

int sdrhip_baudot_process(sdrhip_baudot *h, const uint8_t *bits_host, size_t bits_stride, const uint32_t *counts_host,
                          uint8_t *text_host, size_t text_stride, uint32_t *out_counts_host) {
  return guarded([&] {
    Range roctx_range("sdrhip_baudot_process");
    use_handle(h);
    SDRHIP_REQUIRE(counts_host && text_host && out_counts_host, SDRHIP_E_INVALID, "NULL buffer");
    sdrhip_ctx *ctx = h->ctx;
    const size_t C = (size_t)h->C, cap = h->cap;
    if (bits_stride == 0) bits_stride = h->max_bits;
    if (text_stride == 0) text_stride = cap;
    SDRHIP_REQUIRE(text_stride >= cap, SDRHIP_E_SIZE, "text_stride %zu < capacity %zu of max_bits %zu", text_stride, cap, h->max_bits);
    // the rows are packed on the host first: row c contributes its own count of bytes, none behind it is looked at
    size_t m = 1;
    for (size_t c = 0; c < C; c++) m = std::max(m, std::min((size_t)counts_host[c], h->max_bits));
    h->host_bits.assign(C * m, 0);
    for (size_t c = 0; c < C; c++) {
      const size_t n = std::min((size_t)counts_host[c], h->max_bits);
      if (n) {
        SDRHIP_REQUIRE(bits_host, SDRHIP_E_INVALID, "NULL buffer");
        memcpy(h->host_bits.data() + c * m, bits_host + c * bits_stride, n);
      }
    }
    if (h->st_bits.n < C * m) h->st_bits.alloc(C * m);
    if (!h->st_text.p) { h->st_text.alloc(C * cap); h->st_counts.alloc(C); h->st_outc.alloc(C); }
    SDRHIP_CHECK_HIP(hipMemcpyAsync(h->st_bits.p, h->host_bits.data(), C * m, hipMemcpyHostToDevice, ctx->stream));
    SDRHIP_CHECK_HIP(hipMemcpyAsync(h->st_counts.p, counts_host, C * sizeof(unsigned), hipMemcpyHostToDevice, ctx->stream));
    h->st_text.zero(ctx->stream);   // the bytes of a row behind out_counts[c] reach the caller as zeros
    h->launch(h->st_bits.p, m, h->st_counts.p, h->st_text.p, cap, h->st_outc.p, nullptr);
    unsigned clamped = 0;
    SDRHIP_CHECK_HIP(hipMemcpyAsync(out_counts_host, h->st_outc.p, C * sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    SDRHIP_CHECK_HIP(hipMemcpyAsync(&clamped, h->status.p, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    copy_d2h_rows(ctx, text_host, text_stride, h->st_text.p, cap, cap, C);
    SDRHIP_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    SDRHIP_REQUIRE(!clamped, SDRHIP_E_SIZE, "a row's count exceeds max_bits %zu: clamped, the text is that of the first max_bits half-bits",
                   h->max_bits);
  });
}

int sdrhip_baudot_set_channel(sdrhip_baudot *h, int channel, int stop) {
  return guarded([&] {
    require_channel(h, channel);
    SDRHIP_REQUIRE(bd_stop_ok(stop), SDRHIP_E_INVALID, "stop %d is none of STOP1, STOP15, STOP2", stop);
    h->ctx->use();
    const BdRegs fresh = {0, 0, 0};
    const unsigned letters = SDRHIP_BAUDOT_LETTERS;
    replace_row(h->ctx, h->stops_dev.p + channel, h->stops[channel], stop, h->regs.p + channel, &fresh, sizeof fresh);
    put_sync(h->ctx, h->mode.p + channel, &letters, sizeof letters);
  });
}

int sdrhip_baudot_set_enabled(sdrhip_baudot *h, int channel, int enabled) {
  return guarded([&] {
    require_channel(h, channel);
    h->ctx->use();
    const int v = enabled != 0;
    put_sync(h->ctx, h->en_dev.p + channel, &v, sizeof(int));
    h->enabled[channel] = v;
  });
}

int sdrhip_baudot_get_channels(sdrhip_baudot *h, int *stops, int *enabled, int n) {
  return guarded([&] {
    SDRHIP_REQUIRE(h, SDRHIP_E_INVALID, "handle is NULL");
    SDRHIP_REQUIRE(n >= h->C, SDRHIP_E_SIZE, "n %d < channels %d", n, h->C);
    for (int c = 0; c < h->C; c++) {
      if (stops) stops[c] = h->stops[c];
      if (enabled) enabled[c] = h->enabled[c];
    }
  });
}

int sdrhip_baudot_reset(sdrhip_baudot *h, int keep_mode) {
  return guarded([&] {
    use_handle(h);
    h->reset_rows(0, h->C, keep_mode);
  });
}

int sdrhip_baudot_reset_channel(sdrhip_baudot *h, int channel, int keep_mode) {
  return guarded([&] {
    require_channel(h, channel);
    h->ctx->use();
    h->reset_rows(channel, 1, keep_mode);
  });
}

int sdrhip_baudot_channel_state(sdrhip_baudot *h, int channel, uint16_t *bitstream, uint64_t *bitcount, int *mode) {
  return guarded([&] {
    require_channel(h, channel);
    h->ctx->use();
    BdRegs s;
    unsigned m = 0;
    get_sync(h->ctx, &s, h->regs.p + channel, sizeof s);
    get_sync(h->ctx, &m, h->mode.p + channel, sizeof m);
    if (bitstream) *bitstream = (uint16_t)s.bitstream;
    if (bitcount) *bitcount = s.bitcount;
    if (mode) *mode = (int)m;
  });
}

int sdrhip_baudot_set_channel_state(sdrhip_baudot *h, int channel, uint16_t bitstream, uint64_t bitcount, int mode) {
  return guarded([&] {
    require_channel(h, channel);
    SDRHIP_REQUIRE(mode == SDRHIP_BAUDOT_LETTERS || mode == SDRHIP_BAUDOT_FIGURES, SDRHIP_E_INVALID, "mode %d is neither LETTERS nor FIGURES", mode);
    h->ctx->use();
    const BdRegs s = {bitcount, bitstream, 0};
    const unsigned m = (unsigned)mode;
    put_sync(h->ctx, h->regs.p + channel, &s, sizeof s);
    put_sync(h->ctx, h->mode.p + channel, &m, sizeof m);
  });
}

int sdrhip_baudot_kernel_names(sdrhip_baudot *h, char *buf, size_t len) {
  return guarded([&] {
    write_names(h, buf, len, [] { return "baudot_decode_kernel"; });
  });
}

int sdrhip_baudot_destroy(sdrhip_baudot *h) {
  return guarded([&] { destroy_handle(h); });
}

}  // extern "C"
