// pocsag.hip — the POCSAG decoder bank (sdrhip_pocsag.h): `channels` reference POCSAG nodes (src/pocsag.cc:41-95), one wave of
// 64 lanes per channel, one launch per call. The reference runs pocsag_repair (src/bch31_21.cc:123-212, a brute-force search
// over every 1- and 2-bit error pattern) on the 32-bit window behind EVERY bit while it waits for a sync word. Two facts
// ("POCSAG decoder bank") make that a few instructions per bit:
//   1. the code is BCH(31,21) + even parity, minimum distance 6: error patterns of weight <= 2 have distinct 11-bit syndromes,
//      so pocsag_repair is one look-up in a 2048-entry table with 529 live entries;
//   2. the sync word is a codeword, so "repair(w) == 0 and w == sync" holds exactly when popcount(w ^ sync) <= 2.
#include "sdrhip_internal.hpp"
#include "sdrhip_pocsag.h"
#include "entry.hpp"

using namespace sdrhip;

namespace {

constexpr unsigned POC_SYNC = 0x7CD215D8u;
constexpr unsigned POC_NO_REPAIR = 0xFFFFFFFFu;   // a table entry that no error pattern of weight <= 2 has (those have weight <= 2)
constexpr int POC_CHANNELS_MAX = 8192;
constexpr size_t POC_BITS_MAX = 65536;

// the reference node's protected members, one per channel
struct PocState {
  unsigned long long shift;   // _bits
  unsigned state, bitcount, slot, pad_;
};

// The 11-bit syndrome pocsag_syndrome computes: the remainder of bits 31..1 by g(x) = 0o3551, bit 10 set on odd parity of
// the whole word.
__host__ __device__ inline unsigned poc_syndrome(unsigned w, unsigned odd) {
  unsigned sh = w >> 1;
#pragma unroll
  for (int i = 0; i < 21; i++)
    if (sh & (1u << (30 - i))) sh ^= 03551u << (20 - i);
  return sh | (odd << 10);
}

struct PocArgs {
  const uint8_t *bits; long bits_stride; const unsigned *counts;
  uint2 *events; long ev_stride; unsigned *ev_counts; unsigned *status;
  PocState *st; const int *enabled; const unsigned *table;
  unsigned max_bits;
};

// One block of one wave per channel, so everything but the lane's own window is uniform. The row's bits are packed MSB first
// behind the 64 carried ones: stream bit q sits in W[q / 32] at bit 31 - q % 32, and call bit p is stream bit p + 64. After
// call bit p the reference's _bits holds stream bits p+1 ... p+64.
__global__ __launch_bounds__(64) void pocsag_decode_kernel(PocArgs a) {
  extern __shared__ unsigned W[];   // 2 + 2 * ceil(max_bits / 64) + 1 words
  const unsigned c = blockIdx.x, lane = threadIdx.x;
  if (!a.enabled[c]) {
    if (lane == 0) a.ev_counts[c] = 0;
    return;
  }
  unsigned n = a.counts[c];
  if (n > a.max_bits) {
    n = a.max_bits;
    if (lane == 0) *a.status = 1;
  }
  const PocState s = a.st[c];
  const uint8_t *row = a.bits + (long)c * a.bits_stride;
  const unsigned chunks = (n + 63) >> 6;
  if (lane == 0) { W[0] = (unsigned)(s.shift >> 32); W[1] = (unsigned)s.shift; W[2 + 2 * chunks] = 0; }
  for (unsigned k = 0; k < chunks; k++) {
    const unsigned p = k * 64 + lane;
    const int bit = p < n ? (row[p] & 1) : 0;
    const unsigned long long r = __brevll(__ballot(bit));   // lane 0's bit on top
    if (lane == 0) { W[2 + 2 * k] = (unsigned)(r >> 32); W[3 + 2 * k] = (unsigned)r; }
  }
  __syncthreads();
  // the 32 stream bits from s on; reads W[s / 32 + 1] too, which the pad word covers at the row's end
  auto win = [&](unsigned q) -> unsigned {
    const unsigned long long v = ((unsigned long long)W[q >> 5] << 32) | W[(q >> 5) + 1];
    return (unsigned)(v >> (32 - (q & 31)));
  };

  unsigned state = s.state, bc = s.bitcount, slot = s.slot, p = 0, nev = 0;
  uint2 *ev = a.events + (long)c * a.ev_stride;
  while (p < n) {
    if (state == SDRHIP_POCSAG_WAIT) {
      // 64 positions at a time: the first whose window is within 2 bits of the sync word
      const unsigned q = p + lane;
      const bool hit = q < n && __popc(win(q + 33) ^ POC_SYNC) <= 2;
      const unsigned long long m = __ballot(hit);
      if (m) {
        const unsigned f = (unsigned)__ffsll((long long)m) - 1;
        if (lane == 0 && (long)nev < a.ev_stride) ev[nev] = make_uint2(POC_SYNC, SDRHIP_POCSAG_SYNC | ((p + f) << 8));
        nev++;
        state = SDRHIP_POCSAG_RECEIVE; bc = 0; slot = 0;
        p += f + 1;
      } else p += 64;
      continue;
    }
    // RECEIVE or CHECK_CONTINUE: the rest of this batch. Slot k completes at call bit e0 + 64 (k - slot), the continuation
    // window 32 bits behind slot 7's. Lanes 0..15 take the batch's 16 codewords, lane 16 the continuation window.
    const bool rx = state == SDRHIP_POCSAG_RECEIVE;
    const unsigned e0 = p + 63 - bc;
    const unsigned ec = rx ? e0 + 64 * (7 - slot) + 32 : p + 31 - bc;
    bool has = false;
    unsigned w = 0, info = 0;
    if (lane < 16) {
      const unsigned sl = lane >> 1;
      if (rx && sl >= slot) {
        const unsigned e = e0 + 64 * (sl - slot);
        if (e < n) {
          const unsigned r = win(e + 1 + 32 * (lane & 1));
          const unsigned pat = a.table[poc_syndrome(r, __popc(r) & 1)];
          if (pat != POC_NO_REPAIR) {
            has = true;
            w = r ^ pat;
            info = SDRHIP_POCSAG_WORD | (sl << 2) | (pat ? 32u : 0u) | (e << 8);
          }
        }
      }
    } else if (lane == 16 && ec < n) {
      if (__popc(win(ec + 33) ^ POC_SYNC) > 2) { has = true; info = SDRHIP_POCSAG_END | (ec << 8); }
    }
    const unsigned long long m = __ballot(has);
    const unsigned at = nev + (unsigned)__popcll(m & ((1ull << lane) - 1));
    if (has && (long)at < a.ev_stride) ev[at] = make_uint2(w, info);
    nev += (unsigned)__popcll(m);
    if (ec < n) {   // the continuation check was made within this call
      if ((m >> 16) & 1) { state = SDRHIP_POCSAG_WAIT; bc = 32; slot = 8; }
      else { state = SDRHIP_POCSAG_RECEIVE; bc = 0; slot = 0; }
      p = ec + 1;
    } else {        // the call ends inside the batch
      const unsigned total = bc + (n - p);
      if (!rx) bc = total;
      else if (slot + (total >> 6) >= 8) { bc = total - 64 * (8 - slot); slot = 8; state = SDRHIP_POCSAG_CHECK_CONTINUE; }
      else { slot += total >> 6; bc = total & 63; }
      p = n;
    }
  }
  if (lane == 0) {
    PocState o;
    o.shift = ((unsigned long long)win(n) << 32) | win(n + 32);
    o.state = state; o.bitcount = bc; o.slot = slot; o.pad_ = 0;
    a.st[c] = o;
    a.ev_counts[c] = (long)nev < a.ev_stride ? nev : (unsigned)a.ev_stride;
  }
}

}  // namespace

struct sdrhip_pocsag {
  sdrhip_ctx *ctx = nullptr;
  int C = 1;
  size_t max_bits = 0, cap = 0;   // cap: sdrhip_pocsag_out_capacity(max_bits), the smallest event-row stride
  std::vector<int> enabled;
  DevBuf<int> en_dev;
  DevBuf<PocState> st;
  DevBuf<unsigned> table, status;
  // the host-pointer call's two sides, grown by the calls that need them
  std::vector<uint8_t> host_bits;
  DevBuf<uint8_t> st_bits;
  DevBuf<unsigned> st_counts, st_evc;
  DevBuf<uint2> st_ev;

  void launch(const uint8_t *bits_dev, size_t bits_stride, const unsigned *counts_dev, unsigned *events_dev, size_t ev_stride,
              unsigned *ev_counts_dev, unsigned *status_dev) {
    SDRHIP_REQUIRE(bits_dev && counts_dev && events_dev && ev_counts_dev, SDRHIP_E_INVALID, "NULL buffer");
    if (bits_stride == 0) bits_stride = max_bits;
    if (ev_stride == 0) ev_stride = cap;
    SDRHIP_REQUIRE(ev_stride >= cap, SDRHIP_E_SIZE, "ev_stride %zu < capacity %zu of max_bits %zu", ev_stride, cap, max_bits);
    if (!status_dev) status_dev = status.p;
    SDRHIP_CHECK_HIP(hipMemsetAsync(status_dev, 0, sizeof(unsigned), ctx->stream));
    PocArgs a;
    a.bits = bits_dev; a.bits_stride = (long)bits_stride; a.counts = counts_dev;
    a.events = reinterpret_cast<uint2 *>(events_dev); a.ev_stride = (long)ev_stride; a.ev_counts = ev_counts_dev; a.status = status_dev;
    a.st = st.p; a.enabled = en_dev.p; a.table = table.p; a.max_bits = (unsigned)max_bits;
    const size_t lds = (2 + 2 * ceil_div(max_bits, (size_t)64) + 1) * sizeof(unsigned);
    hipLaunchKernelGGL(pocsag_decode_kernel, dim3((unsigned)C), dim3(64), lds, ctx->stream, a);
    SDRHIP_CHECK_HIP(hipGetLastError());
  }
};

extern "C" {

size_t sdrhip_pocsag_out_capacity(size_t n_bits) { return n_bits / 32 + n_bits / 256 + 4; }

int sdrhip_pocsag_create(sdrhip_ctx *ctx, const int *enabled, int channels, size_t max_bits, sdrhip_pocsag **out) {
  return guarded([&] {
    if (out) *out = nullptr;
    SDRHIP_REQUIRE(enabled && out, SDRHIP_E_INVALID, "NULL argument");
    require_channels(channels, POC_CHANNELS_MAX);
    SDRHIP_REQUIRE(max_bits >= 1 && max_bits <= POC_BITS_MAX, SDRHIP_E_SIZE, "max_bits %zu outside [1,%zu]", max_bits, POC_BITS_MAX);
    require_device_for_null_ctx(ctx);
    make_handle(ctx, out, true, [&](sdrhip_pocsag *h) {
      h->C = channels; h->max_bits = max_bits; h->cap = sdrhip_pocsag_out_capacity(max_bits);
      h->enabled.resize((size_t)channels);
      for (int c = 0; c < channels; c++) h->enabled[c] = enabled[c] != 0;
      // syndrome -> the one error pattern of weight <= 2 that has it: 1 clean, 32 single, 496 double entries
      std::vector<unsigned> table(2048, POC_NO_REPAIR);
      table[0] = 0;
      for (int i = 0; i < 32; i++)
        for (int j = i; j < 32; j++) {
          const unsigned e = (1u << i) | (1u << j);
          table[poc_syndrome(e, (unsigned)__builtin_popcount(e) & 1u)] = e;
        }
      h->table.alloc(table.size());
      h->table.upload(table.data(), table.size(), ctx->stream);
      h->en_dev.alloc((size_t)channels);
      h->en_dev.upload(h->enabled.data(), h->enabled.size(), ctx->stream);
      h->st.alloc((size_t)channels);
      h->st.zero(ctx->stream);
      h->status.alloc(1);
      h->status.zero(ctx->stream);
    });
  });
}

int sdrhip_pocsag_process_dev(sdrhip_pocsag *h, const uint8_t *bits_dev, size_t bits_stride, const uint32_t *counts_dev,
                              uint32_t *events_dev, size_t ev_stride, uint32_t *ev_counts_dev, uint32_t *status_dev) {
  return guarded([&] {
    Range roctx_range("sdrhip_pocsag_process_dev");
    use_handle(h);
    h->launch(bits_dev, bits_stride, counts_dev, events_dev, ev_stride, ev_counts_dev, status_dev);
  });
}

int sdrhip_pocsag_process(sdrhip_pocsag *h, const uint8_t *bits_host, size_t bits_stride, const uint32_t *counts_host,
                          uint32_t *events_host, size_t ev_stride, uint32_t *ev_counts_host) {
  return guarded([&] {
    Range roctx_range("sdrhip_pocsag_process");
    use_handle(h);
    SDRHIP_REQUIRE(counts_host && events_host && ev_counts_host, SDRHIP_E_INVALID, "NULL buffer");
    sdrhip_ctx *ctx = h->ctx;
    const size_t C = (size_t)h->C, cap = h->cap;
    if (bits_stride == 0) bits_stride = h->max_bits;
    if (ev_stride == 0) ev_stride = cap;
    SDRHIP_REQUIRE(ev_stride >= cap, SDRHIP_E_SIZE, "ev_stride %zu < capacity %zu of max_bits %zu", ev_stride, cap, h->max_bits);
    // the rows are packed on the host first: row c contributes its own count of bytes, none behind it is looked at
    size_t m = 1;
    for (size_t c = 0; c < C; c++) m = std::max(m, std::min((size_t)counts_host[c], h->max_bits));
    SDRHIP_REQUIRE(m == 1 || bits_host, SDRHIP_E_INVALID, "NULL buffer");
    h->host_bits.assign(C * m, 0);
    for (size_t c = 0; c < C; c++) {
      const size_t n = std::min((size_t)counts_host[c], h->max_bits);
      if (n) {
        SDRHIP_REQUIRE(bits_host, SDRHIP_E_INVALID, "NULL buffer");
        memcpy(h->host_bits.data() + c * m, bits_host + c * bits_stride, n);
      }
    }
    if (h->st_bits.n < C * m) h->st_bits.alloc(C * m);
    if (!h->st_ev.p) { h->st_ev.alloc(C * cap); h->st_counts.alloc(C); h->st_evc.alloc(C); }
    SDRHIP_CHECK_HIP(hipMemcpyAsync(h->st_bits.p, h->host_bits.data(), C * m, hipMemcpyHostToDevice, ctx->stream));
    SDRHIP_CHECK_HIP(hipMemcpyAsync(h->st_counts.p, counts_host, C * sizeof(unsigned), hipMemcpyHostToDevice, ctx->stream));
    h->st_ev.zero(ctx->stream);   // the events of a row behind ev_counts[c] reach the caller as zeros
    h->launch(h->st_bits.p, m, h->st_counts.p, reinterpret_cast<unsigned *>(h->st_ev.p), cap, h->st_evc.p, nullptr);
    unsigned clamped = 0;
    SDRHIP_CHECK_HIP(hipMemcpyAsync(ev_counts_host, h->st_evc.p, C * sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    SDRHIP_CHECK_HIP(hipMemcpyAsync(&clamped, h->status.p, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    copy_d2h_rows(ctx, events_host, ev_stride * sizeof(uint2), h->st_ev.p, cap * sizeof(uint2), cap * sizeof(uint2), C);
    SDRHIP_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    SDRHIP_REQUIRE(!clamped, SDRHIP_E_SIZE, "a row's count exceeds max_bits %zu: clamped, the events are those of the first max_bits bits",
                   h->max_bits);
  });
}

int sdrhip_pocsag_set_enabled(sdrhip_pocsag *h, int channel, int enabled) {
  return guarded([&] {
    require_channel(h, channel);
    h->ctx->use();
    const int v = enabled != 0;
    put_sync(h->ctx, h->en_dev.p + channel, &v, sizeof(int));
    h->enabled[channel] = v;
  });
}

int sdrhip_pocsag_get_enabled(sdrhip_pocsag *h, int *enabled, int n) {
  return guarded([&] {
    SDRHIP_REQUIRE(h && enabled, SDRHIP_E_INVALID, "NULL argument");
    SDRHIP_REQUIRE(n >= h->C, SDRHIP_E_SIZE, "n %d < channels %d", n, h->C);
    for (int c = 0; c < h->C; c++) enabled[c] = h->enabled[c];
  });
}

int sdrhip_pocsag_reset(sdrhip_pocsag *h) {
  return guarded([&] {
    use_handle(h);
    h->st.zero(h->ctx->stream);
  });
}

int sdrhip_pocsag_reset_channel(sdrhip_pocsag *h, int channel) {
  return guarded([&] {
    require_channel(h, channel);
    h->ctx->use();
    SDRHIP_CHECK_HIP(hipMemsetAsync(h->st.p + channel, 0, sizeof(PocState), h->ctx->stream));
  });
}

int sdrhip_pocsag_channel_state(sdrhip_pocsag *h, int channel, int *state, int *bitcount, int *slot, uint64_t *shift64) {
  return guarded([&] {
    require_channel(h, channel);
    h->ctx->use();
    PocState s;
    get_sync(h->ctx, &s, h->st.p + channel, sizeof(PocState));
    if (state) *state = (int)s.state;
    if (bitcount) *bitcount = (int)s.bitcount;
    if (slot) *slot = (int)s.slot;
    if (shift64) *shift64 = s.shift;
  });
}

int sdrhip_pocsag_kernel_names(sdrhip_pocsag *h, char *buf, size_t len) {
  return guarded([&] {
    write_names(h, buf, len, [] { return "pocsag_decode_kernel"; });
  });
}

int sdrhip_pocsag_destroy(sdrhip_pocsag *h) {
  return guarded([&] { destroy_handle(h); });
}

}  // extern "C"
