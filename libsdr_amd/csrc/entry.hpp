// entry.hpp — the contract of the C entry points around a node handle (create / process_dev / process / reset / destroy),
// written once. Host only; every helper runs inside the entry point's guarded() and reports through SDRHIP_REQUIRE.
// A handle type H has `sdrhip_ctx *ctx` and, for call_begin, `size_t max_in`.
#pragma once
#include "sdrhip_internal.hpp"

namespace sdrhip {

// ---- handle lifetime ---------------------------------------------------------------------------------------------------
// init(h) holds the node's own argument checks (first: nothing is allocated on the device before them) and fills the
// handle; a failure anywhere deletes it, so a handle that owns another one releases it in its destructor. `others`: the
// node's further pointer arguments, non-NULL.
template <class H, class Init>
static inline void make_handle(sdrhip_ctx *ctx, H **out, bool others, Init &&init) {
  SDRHIP_REQUIRE(ctx && out && others, SDRHIP_E_INVALID, "NULL argument");
  *out = nullptr;
  ctx->use();
  H *h = new H;
  try {
    h->ctx = ctx;
    init(h);
    SDRHIP_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  } catch (...) { delete h; throw; }
  *out = h;
}

template <class H>
static inline void destroy_handle(H *h) {
  if (!h) return;
  h->ctx->use();
  (void)hipStreamSynchronize(h->ctx->stream);   // launches in flight still use the handle's buffers
  delete h;
}

// reset / set_*: a live handle on its device
template <class H>
static inline void use_handle(H *h) {
  SDRHIP_REQUIRE(h, SDRHIP_E_INVALID, "handle is NULL");
  h->ctx->use();
}

// ---- argument rules of create ------------------------------------------------------------------------------------------
static inline void require_channels(int channels, int cap) {
  SDRHIP_REQUIRE(channels >= 1 && channels <= cap, SDRHIP_E_INVALID, "channels %d outside [1,%d]", channels, cap);
}
static inline void require_max_in(size_t max_in) {
  SDRHIP_REQUIRE(max_in >= 1 && max_in < (size_t(1) << 30), SDRHIP_E_SIZE, "max_in %zu outside [1,2^30)", max_in);
}

// A create call that checks its argument rules BEFORE the context (host rules: a caller can learn them on a machine without
// a device) ends them with this: where no device exists there is no context to pass — say that, not "NULL argument".
static inline void require_device_for_null_ctx(sdrhip_ctx *ctx) {
  if (ctx) return;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
    (void)hipGetLastError();
    SDRHIP_FAIL(SDRHIP_E_NODEVICE, "no HIP device available, hence no context; libsdrhip has no CPU fallback");
  }
}

// ---- the head of a process / process_dev call ----------------------------------------------------------------------------
// In this order: handle, n against max_in, the empty call (false: nothing to do, and nothing else is looked at), buffers.
// n_name: what the header calls the count ("n", "n_in") — it appears in the messages.
template <class H>
static inline bool call_begin(const H *h, const char *n_name, size_t n, const void *in, const void *out) {
  SDRHIP_REQUIRE(h, SDRHIP_E_INVALID, "handle is NULL");
  SDRHIP_REQUIRE(n <= h->max_in, SDRHIP_E_SIZE, "%s %zu > max_in %zu", n_name, n, h->max_in);
  if (n == 0) return false;
  SDRHIP_REQUIRE(in && out, SDRHIP_E_INVALID, "NULL buffer");
  return true;
}

// Row strides in elements: 0 means packed (in: n, out: the call's output row, which only the node knows). Which checks a
// node makes here is the call site's to say — the copies differed, and the differences are part of the ABI's behaviour:
enum : unsigned {
  STRIDES_TOGETHER = 1,   // one check of both, "stride smaller than <n_name>"
  STRIDE_IN = 2,          // "in_stride a < <n_name> b"
  STRIDE_OUT = 4,         // "out_stride a < <out_name> b" (where absent, launch() makes this check)
};
struct Strides { size_t in, out; };
static inline Strides call_strides(const char *n_name, size_t n, size_t in_stride, size_t out_row, size_t out_stride, unsigned checks,
                            const char *out_name = "outputs") {
  if (in_stride == 0) in_stride = n;
  if (out_stride == 0) out_stride = out_row;
  if (checks & STRIDES_TOGETHER)
    SDRHIP_REQUIRE(in_stride >= n && out_stride >= out_row, SDRHIP_E_SIZE, "stride smaller than %s", n_name);
  if (checks & STRIDE_IN) SDRHIP_REQUIRE(in_stride >= n, SDRHIP_E_SIZE, "in_stride %zu < %s %zu", in_stride, n_name, n);
  if (checks & STRIDE_OUT)
    SDRHIP_REQUIRE(out_stride >= out_row, SDRHIP_E_SIZE, "out_stride %zu < %s %zu", out_stride, out_name, out_row);
  return {in_stride, out_stride};
}

// ---- host-pointer calls: staged through packed device rows -------------------------------------------------------------
struct Staging { DevBuf<uint8_t> in, out; };   // allocated by the first host-pointer call, for the plan's largest one

struct HostIn { const void *p; size_t pitch_b, row_b, rows; };       // the caller's rows; staged packed (pitch = row_b)
struct HostOut { void *p; size_t pitch_b, stage_pitch_b, rows; };    // stage_pitch_b: the row pitch launch writes with
// launch(in_dev, out_dev) runs the node on the staging buffers — with whatever the node needs around its launch — and
// returns the bytes per output row that go back to the caller.
template <class Launch>
static inline void run_staged(sdrhip_ctx *ctx, Staging &st, size_t in_cap_b, size_t out_cap_b, const HostIn &in, const HostOut &out,
                       Launch &&launch) {
  ctx->use();
  if (!st.in.p) { st.in.alloc(in_cap_b); st.out.alloc(out_cap_b); }
  copy_h2d_rows(ctx, st.in.p, in.row_b, in.p, in.pitch_b, in.row_b, in.rows);
  const size_t row_b = launch(st.in.p, st.out.p);
  copy_d2h_rows(ctx, out.p, out.pitch_b, st.out.p, out.stage_pitch_b, row_b, out.rows);
  SDRHIP_CHECK_HIP(hipStreamSynchronize(ctx->stream));
}

// The host-pointer call of a node that writes up to capacity(n) elements per row and says in counts[c] how many: the head
// checks the counts pointer with the handle, an empty call still zeroes the caller's counts, the staged output is zeroed
// first (the elements of a row behind counts[c] reach the caller as zeros) and the counts come back with the rows. H also
// has `int C`, `capacity(n)`, `DevBuf<uint32_t> counts` and `Staging stage`; launch(in_dev, out_dev, cap) runs the node on
// packed rows with h->counts.p. in_elem_b, out_elem_b: the bytes of one input / output element (the strides count elements).
template <class H, class Launch>
static inline void process_counted(H *h, const void *in_host, size_t n, size_t in_stride, size_t in_elem_b, uint8_t *out_host,
                                   size_t out_stride, uint32_t *counts_host, Launch &&launch, size_t out_elem_b = 1) {
  SDRHIP_REQUIRE(h && counts_host, SDRHIP_E_INVALID, "NULL argument");
  if (!call_begin(h, "n", n, in_host, out_host)) { memset(counts_host, 0, (size_t)h->C * sizeof(uint32_t)); return; }
  const size_t cap = h->capacity(n), C = (size_t)h->C, eb = in_elem_b, ob = out_elem_b, out_cap_b = C * h->capacity(h->max_in) * ob;
  const Strides s = call_strides("n", n, in_stride, cap, out_stride, STRIDE_IN | STRIDE_OUT, "capacity");
  // (where a set_channel can raise the capacity of max_in, the staged rows grow with it)
  if (h->stage.out.p && h->stage.out.n < out_cap_b) h->stage.out.alloc(out_cap_b);
  run_staged(h->ctx, h->stage, C * h->max_in * eb, out_cap_b, {in_host, s.in * eb, n * eb, C}, {out_host, s.out * ob, cap * ob, C},
             [&](void *in, void *out) {
               h->stage.out.zero(h->ctx->stream);
               launch(in, static_cast<uint8_t *>(out), cap);
               SDRHIP_CHECK_HIP(hipMemcpyAsync(counts_host, h->counts.p, C * sizeof(uint32_t), hipMemcpyDeviceToHost, h->ctx->stream));
               return cap * ob;
             });
}

// ---- per-channel banks: a handle with `int C` rows, and the calls that read or write one of them -------------------------
// The row index of a set_* / get_* call. A call with a rule of its own between the handle's and the range's (a bank-only
// setter says SDRHIP_E_UNSUPPORTED there; a pointer argument is checked together with the handle) keeps its head and ends
// it with the range-only form.
template <class H>
static inline void require_channel_range(const H *h, int channel) {
  SDRHIP_REQUIRE(channel >= 0 && channel < h->C, SDRHIP_E_INVALID, "channel %d outside [0,%d)", channel, h->C);
}
template <class H>
static inline void require_channel(const H *h, int channel) {
  SDRHIP_REQUIRE(h, SDRHIP_E_INVALID, "handle is NULL");
  require_channel_range(h, channel);
}

// A setter's or getter's copy: enqueued on the context's stream, behind the calls already there, and synchronous — the host
// side may be a local of the caller. Both error codes are collected before the first one is raised, so nothing is left in
// flight when the call returns an error.
static inline void copy_sync(sdrhip_ctx *ctx, void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
  const hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, ctx->stream);
  const hipError_t e2 = hipStreamSynchronize(ctx->stream);
  SDRHIP_CHECK_HIP(e);
  SDRHIP_CHECK_HIP(e2);
}
static inline void put_sync(sdrhip_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes) {
  copy_sync(ctx, dst_dev, src_host, bytes, hipMemcpyHostToDevice);
}
static inline void get_sync(sdrhip_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes) {
  copy_sync(ctx, dst_host, src_dev, bytes, hipMemcpyDeviceToHost);
}

// set_channel: a row's parameters are replaced and its state starts afresh — together or not at all. The device's
// parameters are written, then the device's state; if that fails the old parameters (the host copy still has them) go
// back to the device, and the host copy changes last.
template <class P>
static inline void replace_row(sdrhip_ctx *ctx, P *par_dev, P &par_host, const P &par, void *state_dev, const void *state, size_t state_b) {
  put_sync(ctx, par_dev, &par, sizeof par);
  try {
    put_sync(ctx, state_dev, state, state_b);
  } catch (...) {
    (void)hipMemcpyAsync(par_dev, &par_host, sizeof par_host, hipMemcpyHostToDevice, ctx->stream);
    (void)hipStreamSynchronize(ctx->stream);
    throw;
  }
  par_host = par;
}

// ---- what a handle says about its plan -------------------------------------------------------------------------------------
// *_kernel_names where the answer is a fixed string or a choice among some: text() is asked after the handle is checked.
template <class H, class Text>
static inline void write_names(const H *h, char *buf, size_t len, Text &&text) {
  SDRHIP_REQUIRE(h && buf && len, SDRHIP_E_INVALID, "NULL argument");
  snprintf(buf, len, "%s", text());
}

// *_plan_info of a bank with one geometry for every call length: either pointer may be NULL.
template <class H>
static inline void write_tile_plan(const H *h, int *tile_samples, int *channels_per_group, int tile, int group) {
  SDRHIP_REQUIRE(h, SDRHIP_E_INVALID, "handle is NULL");
  if (tile_samples) *tile_samples = tile;
  if (channels_per_group) *channels_per_group = group;
}

}  // namespace sdrhip
