// ax25.hip — the AX.25 deframer bank (sdrhip_ax25.h): `channels` reference AX25 nodes (src/ax25.cc:79-161), one wave of 64 lanes
// per row, AX_WAVES rows per workgroup, one launch per call. The reference's per-bit loop is restated for 64 positions at a
// time:
//   1. a ballot packs the chunk's bits into one word; with the word before it every lane has the 8 bits _bitstream holds at its
//      position and classifies it as flag, abort, stuffed or data — four masks, local to a lane;
//   2. the flags cut the chunk into segments, eleven at most, walked by a wave-uniform loop; a segment entered with _state 1 is
//      live up to its first abort;
//   3. lane r of a live segment picks the r-th set bit of the data mask by popcount bisection and reads its value, a second
//      ballot gives the data bits compacted; behind the bits of the byte under way they are one word from which whole bytes
//      shift out: lane j stores byte j into the row's _rxbuffer in LDS, the running CRC takes them in turn (eight at most);
//   4. at a flag with _state 1, more than two bytes and the good residue the 64 lanes copy the frame from LDS to the row's
//      output and lane 0 writes the event.
// Nothing in it walks a row bit by bit, and no lane indexes a private array.
#include "sdrhip_internal.hpp"
#include "sdrhip_ax25.h"
#include "entry.hpp"

using namespace sdrhip;

namespace {

constexpr int AX_CHANNELS_MAX = 8192;
constexpr size_t AX_BITS_MAX = 65536;
constexpr int AX_WAVES = 4;   // rows per workgroup
constexpr unsigned AX_RX = SDRHIP_AX25_RXBUFFER;
constexpr unsigned AX_CRC_INIT = 0xFFFFu, AX_CRC_GOOD = 0xF0B8u;

// the reference node's protected members but _rxbuffer, one set per row, and the running CRC of rxbuffer[0:len]: derived state
// (with _state 0 it is not looked at before a flag sets it)
struct AxRegs {
  unsigned bitstream, bitbuffer, state, len, crc, pad_[3];
};

struct AxArgs {
  const uint8_t *bits; long bits_stride; const unsigned *counts;
  uint8_t *bytes; long bytes_stride; unsigned *events; long ev_stride; unsigned *frame_counts; unsigned *status;
  AxRegs *regs; uint8_t *rx; const int *enabled;
  unsigned max_bits, channels;
};

// one byte into the reflected CRC-CCITT (polynomial 0x8408), in shifts and exclusive-ors
__host__ __device__ inline unsigned ax_crc_update(unsigned crc, unsigned byte) {
  unsigned d = (byte ^ crc) & 0xFFu;
  d = (d ^ (d << 4)) & 0xFFu;
  return (((d << 8) | (crc >> 8)) ^ (d >> 4) ^ (d << 3)) & 0xFFFFu;
}

// The bits at positions l - (width - 1) ... l of the chunk, the oldest in bit 0. `cur` holds the chunk's positions 0 ... 63 in
// bits 0 ... 63, `prev` the 64 positions before them.
__device__ inline unsigned long long ax_window(unsigned long long prev, unsigned long long cur, unsigned l, unsigned width) {
  const unsigned s = 65 - width + l;   // the window's oldest bit, counted from prev's bit 0
  return s < 64 ? (prev >> s) | (cur << (64 - s)) : cur >> (s - 64);
}

// the position of the r-th set bit of m (r below its population count), by bisection
__device__ inline unsigned ax_select(unsigned long long m, unsigned r) {
  unsigned pos = 0;
#pragma unroll
  for (unsigned width = 32; width; width >>= 1) {
    const unsigned low = (unsigned)__popcll((m >> pos) & ((1ull << width) - 1));
    if (r >= low) {
      r -= low;
      pos += width;
    }
  }
  return pos;
}

// A lane's LDS writes before it, other lanes' reads of them behind it: the wave's DS instructions execute in the order they were
// issued, and this keeps the compiler from moving one across. A row is a wave's, so no workgroup barrier.
__device__ inline void ax_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__global__ __launch_bounds__(64 * AX_WAVES) void ax25_deframe_kernel(AxArgs a) {
  __shared__ unsigned char rx_all[AX_WAVES][AX_RX];
  const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned c = blockIdx.x * AX_WAVES + wave;
  if (c >= a.channels) return;   // (whole waves: a row is a wave's, and nothing below synchronises the workgroup)
  if (!a.enabled[c]) {
    if (lane == 0) a.frame_counts[c] = 0;
    return;
  }
  unsigned n = a.counts[c];
  if (n > a.max_bits) {
    n = a.max_bits;
    if (lane == 0) *a.status = 1;
  }
  if (n == 0) {
    if (lane == 0) a.frame_counts[c] = 0;
    return;
  }
  const AxRegs s = a.regs[c];
  const uint8_t *row = a.bits + (long)c * a.bits_stride;
  uint8_t *bytes = a.bytes + (long)c * a.bytes_stride;
  unsigned *events = a.events + (long)c * a.ev_stride * 2;
  uint8_t *rx_dev = a.rx + (size_t)c * AX_RX;
  unsigned char *rx = rx_all[wave];

  unsigned bitbuffer = s.bitbuffer, state = s.state, len = s.len < AX_RX ? s.len : AX_RX, crc = s.crc;
  for (unsigned i = lane; i < len; i += 64) rx[i] = rx_dev[i];
  ax_wave_sync();

  // carried _bitstream: its bit 0 is position -1, so the bit-reversed word has it in bit 63
  unsigned long long prev = __brevll((unsigned long long)s.bitstream), cur = 0;
  unsigned nframes = 0, nbytes = 0;
  const unsigned chunks = (n + 63) >> 6;
  for (unsigned k = 0; k < chunks; k++) {
    const unsigned base = k * 64, p = base + lane;
    const unsigned m = n - base < 64 ? n - base : 64;   // the chunk's positions
    const bool valid = lane < m;
    const int bit = valid ? (row[p] & 1) : 0;
    if (k) prev = cur;
    cur = __ballot(bit);
    // the class of a position: bit 7 of x is the position itself, bit 0 the one seven before it
    const unsigned x = (unsigned)ax_window(prev, cur, lane, 8) & 0xFFu;
    const unsigned long long F = __ballot(valid && x == 0x7Eu);
    if (!state && !F) continue;   // idle through the whole chunk
    const unsigned long long A = __ballot(valid && (x & 0xFEu) == 0xFEu);
    const unsigned long long S = __ballot(valid && (x & 0xFCu) == 0x7Cu);   // (a flag matches too: F comes first)
    const unsigned long long D = (m == 64 ? ~0ull : (1ull << m) - 1) & ~(F | A | S);
    // the segments: each ends at a flag or at the chunk's end
    for (unsigned start = 0; start < m;) {
      const unsigned long long rest = ~0ull << start, f = F & rest;
      const unsigned end = f ? (unsigned)__ffsll((long long)f) - 1 : m;
      unsigned long long seg = rest & (end == 64 ? ~0ull : (1ull << end) - 1);
      if (state) {
        const unsigned long long ab = A & seg;
        if (ab) seg &= (ab & (0 - ab)) - 1;   // nothing behind the first abort is live
        const unsigned long long dm = D & seg;
        const unsigned kb = 8u - (unsigned)__ffs((int)bitbuffer);   // bits of the byte under way, above the marker
        const unsigned long long part = bitbuffer >> (8 - kb);
        unsigned nd = (unsigned)__popcll(dm);
        const unsigned room = (AX_RX + 1) * 8 - (len * 8 + kb);   // data bits up to and with the one that overflows
        const bool over = nd >= room;
        if (over) nd = room;
        const unsigned pos = ax_select(dm, lane);
        const unsigned long long word = __ballot(lane < nd && ((cur >> pos) & 1));   // the data bits, compacted
        const unsigned long long lo = part | (word << kb), hi = kb ? word >> (64 - kb) : 0;
        const unsigned t = kb + nd, nb = t >> 3;   // nb <= 8: the whole bytes lie in lo
        const unsigned stored = nb < AX_RX - len ? nb : AX_RX - len;
        if (lane < stored) rx[len + lane] = (unsigned char)(lo >> (8 * lane));
        for (unsigned j = 0; j < stored; j++) crc = ax_crc_update(crc, (unsigned)(lo >> (8 * j)) & 0xFFu);
        len += stored;
        if (over) {   // the byte that found no room stays in _bitbuffer, under its marker
          bitbuffer = 1u | (((unsigned)(lo >> (8 * (nb - 1))) & 0xFFu) << 1);
          state = 0;
        } else {
          const unsigned k2 = t & 7, sh = t - k2;
          const unsigned rem = (unsigned)(sh == 64 ? hi : lo >> sh) & ((1u << k2) - 1);
          bitbuffer = (0x80u >> k2) | (rem << (8 - k2));
          if (ab) state = 0;
        }
      }
      if (end < m) {   // the flag
        if (state && len > 2 && crc == AX_CRC_GOOD) {
          const unsigned flen = len - 2;
          ax_wave_sync();   // single lanes wrote the bytes, all lanes read them
          for (unsigned i = lane; i < flen; i += 64)
            if ((long)(nbytes + i) < a.bytes_stride) bytes[nbytes + i] = rx[i];
          if (lane == 0 && (long)nframes < a.ev_stride) {
            events[2 * nframes] = nbytes;
            events[2 * nframes + 1] = flen | ((base + end) << 16);
          }
          ax_wave_sync();   // the reads before the next frame's writes
          nbytes += flen;
          nframes++;
        }
        state = 1;
        len = 0;
        bitbuffer = 0x80u;
        crc = AX_CRC_INIT;
      }
      start = end + 1;
    }
  }
  ax_wave_sync();
  for (unsigned i = lane; i < len; i += 64) rx_dev[i] = rx[i];
  if (lane == 0) {
    AxRegs o;
    o.bitstream = __brev((unsigned)ax_window(prev, cur, (n - 1) & 63, 32));
    o.bitbuffer = bitbuffer; o.state = state; o.len = len; o.crc = crc;
    o.pad_[0] = o.pad_[1] = o.pad_[2] = 0;
    a.regs[c] = o;
    a.frame_counts[c] = (long)nframes < a.ev_stride ? nframes : (unsigned)a.ev_stride;
  }
}

}  // namespace

struct sdrhip_ax25 {
  sdrhip_ctx *ctx = nullptr;
  int C = 1;
  size_t max_bits = 0, fcap = 0, bcap = 0;   // the capacities of max_bits: the smallest event-row and byte-row strides
  std::vector<int> enabled;
  DevBuf<int> en_dev;
  DevBuf<AxRegs> regs;
  DevBuf<uint8_t> rx;   // channels rows of AX_RX: _rxbuffer
  DevBuf<unsigned> status;
  // the host-pointer call's two sides, grown by the calls that need them
  std::vector<uint8_t> host_bits;
  DevBuf<uint8_t> st_bits, st_bytes;
  DevBuf<unsigned> st_counts, st_events, st_fc;

  void strides(size_t &bits_stride, size_t &bytes_stride, size_t &ev_stride) const {
    if (bits_stride == 0) bits_stride = max_bits;
    if (bytes_stride == 0) bytes_stride = bcap;
    if (ev_stride == 0) ev_stride = fcap;
    SDRHIP_REQUIRE(bytes_stride >= bcap, SDRHIP_E_SIZE, "bytes_stride %zu < capacity %zu of max_bits %zu", bytes_stride, bcap, max_bits);
    SDRHIP_REQUIRE(ev_stride >= fcap, SDRHIP_E_SIZE, "ev_stride %zu < capacity %zu of max_bits %zu", ev_stride, fcap, max_bits);
  }
  void launch(const uint8_t *bits_dev, size_t bits_stride, const unsigned *counts_dev, uint8_t *bytes_dev, size_t bytes_stride,
              unsigned *events_dev, size_t ev_stride, unsigned *frame_counts_dev, unsigned *status_dev) {
    SDRHIP_REQUIRE(bits_dev && counts_dev && bytes_dev && events_dev && frame_counts_dev, SDRHIP_E_INVALID, "NULL buffer");
    strides(bits_stride, bytes_stride, ev_stride);
    if (!status_dev) status_dev = status.p;
    SDRHIP_CHECK_HIP(hipMemsetAsync(status_dev, 0, sizeof(unsigned), ctx->stream));
    AxArgs a;
    a.bits = bits_dev; a.bits_stride = (long)bits_stride; a.counts = counts_dev;
    a.bytes = bytes_dev; a.bytes_stride = (long)bytes_stride; a.events = events_dev; a.ev_stride = (long)ev_stride;
    a.frame_counts = frame_counts_dev; a.status = status_dev;
    a.regs = regs.p; a.rx = rx.p; a.enabled = en_dev.p;
    a.max_bits = (unsigned)max_bits; a.channels = (unsigned)C;
    hipLaunchKernelGGL(ax25_deframe_kernel, dim3((unsigned)ceil_div((size_t)C, (size_t)AX_WAVES)), dim3(64 * AX_WAVES), 0, ctx->stream, a);
    SDRHIP_CHECK_HIP(hipGetLastError());
  }
  // config() on `rows` nodes: the registers and _state 0, the buffer empty (its bytes stay, nothing reads them)
  void reset_rows(int first, int rows) { SDRHIP_CHECK_HIP(hipMemsetAsync(regs.p + first, 0, (size_t)rows * sizeof(AxRegs), ctx->stream)); }
};

extern "C" {

size_t sdrhip_ax25_frames_capacity(size_t n_bits) { return n_bits / 25 + 1; }
size_t sdrhip_ax25_bytes_capacity(size_t n_bits) { return n_bits / 8 + AX_RX; }

int sdrhip_ax25_create(sdrhip_ctx *ctx, const int *enabled, int channels, size_t max_bits, sdrhip_ax25 **out) {
  return guarded([&] {
    if (out) *out = nullptr;
    SDRHIP_REQUIRE(out, SDRHIP_E_INVALID, "NULL argument");
    require_channels(channels, AX_CHANNELS_MAX);
    SDRHIP_REQUIRE(max_bits >= 1 && max_bits <= AX_BITS_MAX, SDRHIP_E_SIZE, "max_bits %zu outside [1,%zu]", max_bits, AX_BITS_MAX);
    require_device_for_null_ctx(ctx);
    make_handle(ctx, out, true, [&](sdrhip_ax25 *h) {
      h->C = channels; h->max_bits = max_bits;
      h->fcap = sdrhip_ax25_frames_capacity(max_bits); h->bcap = sdrhip_ax25_bytes_capacity(max_bits);
      h->enabled.resize((size_t)channels);
      for (int c = 0; c < channels; c++) h->enabled[c] = enabled ? enabled[c] != 0 : 1;
      h->en_dev.alloc((size_t)channels);
      h->en_dev.upload(h->enabled.data(), h->enabled.size(), ctx->stream);
      h->regs.alloc((size_t)channels);
      h->regs.zero(ctx->stream);
      h->rx.alloc((size_t)channels * AX_RX);
      h->rx.zero(ctx->stream);
      h->status.alloc(1);
      h->status.zero(ctx->stream);
    });
  });
}

int sdrhip_ax25_process_dev(sdrhip_ax25 *h, const uint8_t *bits_dev, size_t bits_stride, const uint32_t *counts_dev, uint8_t *bytes_dev,
                            size_t bytes_stride, uint32_t *events_dev, size_t ev_stride, uint32_t *frame_counts_dev, uint32_t *status_dev) {
  return guarded([&] {
    Range roctx_range("sdrhip_ax25_process_dev");
    use_handle(h);
    h->launch(bits_dev, bits_stride, counts_dev, bytes_dev, bytes_stride, events_dev, ev_stride, frame_counts_dev, status_dev);
  });
}

int sdrhip_ax25_process(sdrhip_ax25 *h, const uint8_t *bits_host, size_t bits_stride, const uint32_t *counts_host, uint8_t *bytes_host,
                        size_t bytes_stride, uint32_t *events_host, size_t ev_stride, uint32_t *frame_counts_host) {
  return guarded([&] {
    Range roctx_range("sdrhip_ax25_process");
    use_handle(h);
    SDRHIP_REQUIRE(counts_host && bytes_host && events_host && frame_counts_host, SDRHIP_E_INVALID, "NULL buffer");
    sdrhip_ctx *ctx = h->ctx;
    const size_t C = (size_t)h->C, bcap = h->bcap, fcap = h->fcap;
    h->strides(bits_stride, bytes_stride, ev_stride);
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
    if (!h->st_bytes.p) { h->st_bytes.alloc(C * bcap); h->st_events.alloc(C * fcap * 2); h->st_counts.alloc(C); h->st_fc.alloc(C); }
    SDRHIP_CHECK_HIP(hipMemcpyAsync(h->st_bits.p, h->host_bits.data(), C * m, hipMemcpyHostToDevice, ctx->stream));
    SDRHIP_CHECK_HIP(hipMemcpyAsync(h->st_counts.p, counts_host, C * sizeof(unsigned), hipMemcpyHostToDevice, ctx->stream));
    h->st_bytes.zero(ctx->stream);    // what lies behind a row's frames reaches the caller as zeros
    h->st_events.zero(ctx->stream);
    h->launch(h->st_bits.p, m, h->st_counts.p, h->st_bytes.p, bcap, h->st_events.p, fcap, h->st_fc.p, nullptr);
    unsigned clamped = 0;
    SDRHIP_CHECK_HIP(hipMemcpyAsync(frame_counts_host, h->st_fc.p, C * sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    SDRHIP_CHECK_HIP(hipMemcpyAsync(&clamped, h->status.p, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    copy_d2h_rows(ctx, bytes_host, bytes_stride, h->st_bytes.p, bcap, bcap, C);
    copy_d2h_rows(ctx, events_host, ev_stride * 8, h->st_events.p, fcap * 8, fcap * 8, C);
    SDRHIP_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    SDRHIP_REQUIRE(!clamped, SDRHIP_E_SIZE, "a row's count exceeds max_bits %zu: clamped, the frames are those of the first max_bits bits",
                   h->max_bits);
  });
}

int sdrhip_ax25_set_enabled(sdrhip_ax25 *h, int channel, int enabled) {
  return guarded([&] {
    require_channel(h, channel);
    h->ctx->use();
    const int v = enabled != 0;
    put_sync(h->ctx, h->en_dev.p + channel, &v, sizeof(int));
    h->enabled[channel] = v;
  });
}

int sdrhip_ax25_get_enabled(sdrhip_ax25 *h, int *enabled, int n) {
  return guarded([&] {
    SDRHIP_REQUIRE(h && enabled, SDRHIP_E_INVALID, "NULL argument");
    SDRHIP_REQUIRE(n >= h->C, SDRHIP_E_SIZE, "n %d < channels %d", n, h->C);
    for (int c = 0; c < h->C; c++) enabled[c] = h->enabled[c];
  });
}

int sdrhip_ax25_reset(sdrhip_ax25 *h) {
  return guarded([&] {
    use_handle(h);
    h->reset_rows(0, h->C);
  });
}

int sdrhip_ax25_reset_channel(sdrhip_ax25 *h, int channel) {
  return guarded([&] {
    require_channel(h, channel);
    h->ctx->use();
    h->reset_rows(channel, 1);
  });
}

int sdrhip_ax25_channel_state(sdrhip_ax25 *h, int channel, uint32_t *bitstream, uint32_t *bitbuffer, int *state, int *len, uint8_t *rxbuffer) {
  return guarded([&] {
    require_channel(h, channel);
    h->ctx->use();
    AxRegs s;
    get_sync(h->ctx, &s, h->regs.p + channel, sizeof s);
    if (rxbuffer && s.len) get_sync(h->ctx, rxbuffer, h->rx.p + (size_t)channel * AX_RX, std::min(s.len, AX_RX));
    if (bitstream) *bitstream = s.bitstream;
    if (bitbuffer) *bitbuffer = s.bitbuffer;
    if (state) *state = (int)s.state;
    if (len) *len = (int)s.len;
  });
}

int sdrhip_ax25_set_channel_state(sdrhip_ax25 *h, int channel, uint32_t bitstream, uint32_t bitbuffer, int state, int len, const uint8_t *rxbuffer) {
  return guarded([&] {
    require_channel(h, channel);
    SDRHIP_REQUIRE(state == 0 || state == 1, SDRHIP_E_INVALID, "state %d is neither 0 nor 1", state);
    SDRHIP_REQUIRE(len >= 0 && len <= (int)AX_RX, SDRHIP_E_INVALID, "len %d outside [0,%u]", len, AX_RX);
    SDRHIP_REQUIRE(rxbuffer || !len, SDRHIP_E_INVALID, "NULL rxbuffer with len %d", len);
    SDRHIP_REQUIRE(!state || (bitbuffer >= 1 && bitbuffer <= 0xFF), SDRHIP_E_INVALID, "bitbuffer 0x%x outside [1,0xff] with state 1", bitbuffer);
    h->ctx->use();
    AxRegs s = {bitstream, bitbuffer, (unsigned)state, (unsigned)len, AX_CRC_INIT, {0, 0, 0}};
    for (int i = 0; i < len; i++) s.crc = ax_crc_update(s.crc, rxbuffer[i]);
    if (len) put_sync(h->ctx, h->rx.p + (size_t)channel * AX_RX, rxbuffer, (size_t)len);
    put_sync(h->ctx, h->regs.p + channel, &s, sizeof s);
  });
}

int sdrhip_ax25_kernel_names(sdrhip_ax25 *h, char *buf, size_t len) {
  return guarded([&] {
    write_names(h, buf, len, [] { return "ax25_deframe_kernel"; });
  });
}

int sdrhip_ax25_destroy(sdrhip_ax25 *h) {
  return guarded([&] { destroy_handle(h); });
}

}  // extern "C"
