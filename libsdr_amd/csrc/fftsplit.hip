// fftsplit.hip — FilterSink and FilterSource as two stages around a PUBLIC spectrum stream (no rocFFT/hipFFT).
//
// Replaces (reference, file:line):
//   FilterSink<Scalar>::process     src/filternode.hh:81-88   (N samples, zero-padded to 2N, forward FFT, send the spectrum)
//   FilterSource<Scalar>::process   src/filternode.hh:164-181 (spectrum x kernel, inverse FFT, /2N, overlap-ADD the carried tail)
//
// Unlike the fused filter (fftconv.hip, overlap-save, digit-reversed internal spectra) the spectrum here is what the reference
// sends between the two nodes: 2N points per block, natural order, unnormalised forward DFT with the FFTW sign (-1), and the
// source carries the last block's upper half (the tail) from block to block and call to call, as _last_trafo does.
//
// Fused path (complex<float>, 2N a power of two in [2048, 16384]): the radix-16 passes of fft16.hpp, NT = 2N/16 lanes.
//   forward:  one workgroup per (channel, block); pass 0 reads the N samples straight from global memory (its upper 8 inputs
//             per butterfly are the zero half: dft16<.., LOW_HALF>), the other passes run in LDS, and the store walks the
//             NATURAL frequency order, reading the digit-reversed image through a position table (reorder in LDS, coalesced
//             global writes).
//   inverse:  strands: workgroup (strand, channel) walks a run of the channel's consecutive blocks; each block's natural
//             spectrum times the kernel spectrum (natural, pre-scaled by 1/2N) is scattered into LDS in digit-reversed order,
//             the inverse passes run, and out = tail + y[0:N], tail = y[N:2N] with the tail in registers (R = N / NT float2 per
//             lane: 8 on 2N / 16 lanes, 16 on 512 lanes at 2N = 16384 — 1024 lanes there cap a lane at 128 registers, and the
//             tail on top of a radix-16 pass spilled). A strand's first block lacks the previous strand's last tail: fftsplit_fixup_kernel adds it afterwards and
//             moves the channel's last tail into the handle's state (same shape as iqbb_fm_multi_fixup_kernel).
// Composed path (every other size, and complex<double>): the planned transforms (sdrhip_fft_plan_*) between small kernels:
//   gather + pad -> forward transforms -> strided copy into the spectrum rows; spectrum product -> inverse transforms ->
//   overlap-add scatter (one lane per (channel, point) walks the blocks, tail in a register).
#include "sdrhip_internal.hpp"
#include "entry.hpp"

#include <cmath>
#include <memory>
#include <vector>

using namespace sdrhip;

// float tolerance path (<= 1e-5 relative): fused multiply-adds are welcome here
#pragma clang fp contract(fast)

#include "fft16.hpp"

namespace {

// ---- fused complex<float> path --------------------------------------------------------------------------------------
template <int NT>
__global__ __launch_bounds__(NT) void fftsink_fwd_kernel(const FftDev p, const int *pos_of, const float2 *in, long in_stride,
                                                         int N, float2 *spec, long spec_stride) {
  extern __shared__ __attribute__((aligned(16))) float2 xl[];
  const int tid = threadIdx.x, L = p.L, c = blockIdx.y;
  const float2 *src = in + (long)c * in_stride + (long)blockIdx.x * N;
  float2 *dst = spec + (long)c * spec_stride + (long)blockIdx.x * L;
  // pass 0 (radix 16, stride s = L / 16): butterfly j reads points j + k s; k >= 8 lie in the zero half
  const int s = L / 16;
  for (int j = tid; j < s; j += NT) {
    float2 v[16], w[16];
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = src[j + k * s];
    dft16<-1, true>(v);
    twiddles16(p, 0, s, j, w);
#pragma unroll
    for (int k = 1; k < 16; k++) v[k] = cmul(v[k], w[k]);
#pragma unroll
    for (int k = 0; k < 16; k++) xl[PAD(j + k * s)] = v[k];
  }
  __syncthreads();
  dif_passes<NT>(xl, p, tid, 1);
  for (int k = tid; k < L; k += NT) dst[k] = xl[PAD(pos_of[k])];   // natural order out
}

// grid (strands, channels); strand st covers blocks [st bps, min(nb, (st + 1) bps)). tail: the channels' carried state
// (read by strand 0 only), stail: every strand's last tail (channels x nstr x N) for the fix-up
template <int NT, int R>
__global__ __launch_bounds__(NT) void fftsource_inv_kernel(const FftDev p, const int *pos_of, const float2 *K, const float2 *spec,
                                                           long spec_stride, int nb, int bps, const float2 *tail, float2 *stail,
                                                           float2 *out, long out_stride) {
  extern __shared__ __attribute__((aligned(16))) float2 xl[];
  const int tid = threadIdx.x, L = p.L, N = L / 2, c = blockIdx.y, st = blockIdx.x;
  const int b0 = st * bps, b1 = min(nb, b0 + bps);
  float2 t[R];
#pragma unroll
  for (int m = 0; m < R; m++) t[m] = st == 0 ? tail[(long)c * N + tid + m * NT] : make_float2(0.f, 0.f);
  for (int b = b0; b < b1; b++) {
    const float2 *sp = spec + (long)c * spec_stride + (long)b * L;
    for (int k = tid; k < L; k += NT) xl[PAD(pos_of[k])] = cmul(sp[k], K[k]);   // digit-reversed order in
    __syncthreads();
    dit_passes<NT, true>(xl, p, tid);
    float2 *o = out + (long)c * out_stride + (long)b * N;
#pragma unroll
    for (int m = 0; m < R; m++) {
      const int i = tid + m * NT;
      o[i] = cadd(t[m], xl[PAD(i)]);
      t[m] = xl[PAD(N + i)];
    }
    __syncthreads();   // the next block overwrites the image
  }
  float2 *ts = stail + ((long)c * gridDim.x + st) * N;
#pragma unroll
  for (int m = 0; m < R; m++) ts[tid + m * NT] = t[m];
}

// the first block of strand st >= 1 gets strand st - 1's last tail; the last strand's tail becomes the channel's state
template <class T2>
__global__ void fftsplit_fixup_kernel(int N, int nstr, int bps, const T2 *stail, T2 *tail, T2 *out, long out_stride) {
  const int c = blockIdx.y;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
    for (int st = 1; st < nstr; st++) {
      T2 &o = out[(long)c * out_stride + (long)st * bps * N + i];
      const T2 a = stail[((long)c * nstr + st - 1) * N + i];
      o.x += a.x; o.y += a.y;
    }
    tail[(long)c * N + i] = stail[((long)c * nstr + nstr - 1) * N + i];
  }
}

// ---- composed path (any N, complex<float> and complex<double>) --------------------------------------------------------
// X[(c nb + b) L + k] = k < N ? in[c][b N + k] : 0
template <class T2>
__global__ void fftsplit_pad_kernel(const T2 *in, long in_stride, int N, long L, int nb, long total, T2 *X) {
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const long k = e % L, cb = e / L, b = cb % nb, c = cb / nb;
    T2 v; v.x = 0; v.y = 0;
    if (k < N) v = in[c * in_stride + b * N + k];
    X[e] = v;
  }
}
// spec[c][b L + k] = X[(c nb + b) L + k]
template <class T2>
__global__ void fftsplit_rows_kernel(const T2 *X, long row, long total, T2 *spec, long spec_stride) {
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x)
    spec[(e / row) * spec_stride + e % row] = X[e];
}
// Y[(c nb + b) L + k] = spec[c][b L + k] K[k]
template <class T2>
__global__ void fftsplit_mul_kernel(const T2 *spec, long spec_stride, const T2 *K, long L, long row, long total, T2 *Y) {
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const T2 a = spec[(e / row) * spec_stride + e % row], w = K[e % L];
    T2 r; r.x = a.x * w.x - a.y * w.y; r.y = a.x * w.y + a.y * w.x;
    Y[e] = r;
  }
}
// out[c][b N + i] = tail + Y[(c nb + b) L + i]; tail = Y[... + N + i]
template <class T2>
__global__ void fftsplit_ola_kernel(const T2 *Y, int N, long L, int nb, T2 *tail, T2 *out, long out_stride) {
  const int c = blockIdx.y;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
    T2 t = tail[(long)c * N + i];
    for (int b = 0; b < nb; b++) {
      const T2 *y = Y + ((long)c * nb + b) * L;
      T2 o = y[i];
      o.x += t.x; o.y += t.y;
      out[(long)c * out_stride + (long)b * N + i] = o;
      t = y[N + i];
    }
    tail[(long)c * N + i] = t;
  }
}

inline dim3 grid1d(long total) { return dim3((unsigned)std::min<long>((total + 255) / 256, 4096)); }

// what both handles share: sizes, the plan the size takes, staging for the host entry points
struct SplitBase {
  sdrhip_ctx *ctx = nullptr;
  int dtype = SDRHIP_T_CF32, N = 0, L = 0, C = 0;
  size_t max_blocks = 0;
  bool fused = false;
  FftPlan fp;                              // fused: the radix-16 tables
  DevBuf<int> pos_of;                      // fused: frequency -> position in the digit-reversed image
  sdrhip_fft_plan *plan = nullptr;         // composed: the planned L-point transform
  DevBuf<char> scratch;                    // composed: C x max_blocks x L points
  Staging stage;                           // host entry points
  int nt = 0;                              // fused: lanes per workgroup (L / 16)

  size_t elem() const { return dtype == SDRHIP_T_CF64 ? 16 : 8; }
  void build(sdrhip_ctx *ctx_, int dtype_, int N_, int channels, size_t max_blocks_) {
    SDRHIP_REQUIRE(ctx_, SDRHIP_E_INVALID, "context is NULL");
    SDRHIP_REQUIRE(dtype_ == SDRHIP_T_CF32 || dtype_ == SDRHIP_T_CF64, SDRHIP_E_INVALID,
                   "dtype %d: need SDRHIP_T_CF32 or SDRHIP_T_CF64", dtype_);
    SDRHIP_REQUIRE(N_ >= 1 && N_ <= (1 << 26), SDRHIP_E_INVALID, "block size %d: need 1 ... 2^26", N_);
    SDRHIP_REQUIRE(channels >= 1 && channels <= 65535, SDRHIP_E_INVALID, "channels %d", channels);
    SDRHIP_REQUIRE(max_blocks_ >= 1 && max_blocks_ <= (1u << 20), SDRHIP_E_INVALID, "max_blocks %zu", max_blocks_);
    ctx = ctx_; dtype = dtype_; N = N_; L = 2 * N_; C = channels; max_blocks = max_blocks_;
    ctx->use();
    fused = dtype == SDRHIP_T_CF32 && L >= 2048 && L <= 16384 && (L & (L - 1)) == 0;
    if (fused) {
      fp.build(ctx, L);
      std::vector<int> inv(L);
      for (int pos = 0; pos < L; pos++) inv[fp.perm[pos]] = pos;
      pos_of.alloc(L); pos_of.upload(inv.data(), L, ctx->stream);
      nt = L / 16;
    } else {
      const int rc = sdrhip_fft_plan_create(ctx, dtype, L, &plan);
      if (rc != SDRHIP_OK) throw Failure{rc};
      scratch.alloc((size_t)C * max_blocks * L * elem());
    }
  }
  ~SplitBase() { if (plan) sdrhip_fft_plan_destroy(plan); }
  const char *form() const { return fused ? "fused" : "composed"; }
  size_t blocks_of(size_t n_in) const {
    SDRHIP_REQUIRE(n_in % (size_t)N == 0, SDRHIP_E_INVALID, "n_in %zu is not a whole number of %d-sample blocks", n_in, N);
    const size_t nb = n_in / (size_t)N;
    SDRHIP_REQUIRE(nb <= max_blocks, SDRHIP_E_SIZE, "%zu blocks > max_blocks %zu", nb, max_blocks);
    return nb;
  }
  void exec(int sign, int batch, const void *in, void *out) {
    const int rc = sdrhip_fft_plan_exec_dev(plan, sign, batch, in, out);
    if (rc != SDRHIP_OK) throw Failure{rc};
  }
};

#define SDRHIP_SPLIT_NT(KERNEL_, ...) do { switch (h->nt) { \
    case 128: hipLaunchKernelGGL(KERNEL_<128>, __VA_ARGS__); break; \
    case 256: hipLaunchKernelGGL(KERNEL_<256>, __VA_ARGS__); break; \
    case 512: hipLaunchKernelGGL(KERNEL_<512>, __VA_ARGS__); break; \
    default: hipLaunchKernelGGL(KERNEL_<1024>, __VA_ARGS__); break; } } while (0)

}  // namespace

struct sdrhip_fftsink : SplitBase {
  void launch(const void *in, size_t nb, size_t in_stride, void *spec, size_t spec_stride) {
    ctx->use();
    const long Ll = L;
    if (fused) {
      const size_t lds = fp.lds_bytes();
      sdrhip_fftsink *h = this;
      SDRHIP_SPLIT_NT(fftsink_fwd_kernel, dim3((unsigned)nb, (unsigned)C), dim3(nt), lds, ctx->stream, fp.dev, pos_of.p,
                      static_cast<const float2 *>(in), (long)in_stride, N, static_cast<float2 *>(spec), (long)spec_stride);
    } else if (dtype == SDRHIP_T_CF32) {
      float2 *X = reinterpret_cast<float2 *>(scratch.p);
      const long total = (long)C * nb * Ll;
      hipLaunchKernelGGL(fftsplit_pad_kernel<float2>, grid1d(total), dim3(256), 0, ctx->stream, static_cast<const float2 *>(in),
                         (long)in_stride, N, Ll, (int)nb, total, X);
      exec(-1, (int)(C * nb), X, X);
      hipLaunchKernelGGL(fftsplit_rows_kernel<float2>, grid1d(total), dim3(256), 0, ctx->stream, X, (long)nb * Ll, total,
                         static_cast<float2 *>(spec), (long)spec_stride);
    } else {
      double2 *X = reinterpret_cast<double2 *>(scratch.p);
      const long total = (long)C * nb * Ll;
      hipLaunchKernelGGL(fftsplit_pad_kernel<double2>, grid1d(total), dim3(256), 0, ctx->stream, static_cast<const double2 *>(in),
                         (long)in_stride, N, Ll, (int)nb, total, X);
      exec(-1, (int)(C * nb), X, X);
      hipLaunchKernelGGL(fftsplit_rows_kernel<double2>, grid1d(total), dim3(256), 0, ctx->stream, X, (long)nb * Ll, total,
                         static_cast<double2 *>(spec), (long)spec_stride);
    }
    SDRHIP_CHECK_HIP(hipGetLastError());
  }
};

struct sdrhip_fftsource : SplitBase {
  DevBuf<char> K;        // the kernel spectrum, natural order, pre-scaled by 1 / L
  DevBuf<char> tail;     // C x N: the carried upper halves (_last_trafo)
  DevBuf<char> stail;    // fused: C x max strands x N
  int max_str = 0;       // fused: strands per channel at most

  void set_kernel(const void *spectrum) {
    SDRHIP_REQUIRE(spectrum, SDRHIP_E_INVALID, "kernel spectrum is NULL");
    ctx->use();
    std::vector<char> k((size_t)L * elem());
    if (dtype == SDRHIP_T_CF64) {
      const double *s = static_cast<const double *>(spectrum);
      double *d = reinterpret_cast<double *>(k.data());
      for (long i = 0; i < 2L * L; i++) d[i] = s[i] / (double)L;
    } else {
      const float *s = static_cast<const float *>(spectrum);
      float *d = reinterpret_cast<float *>(k.data());
      for (long i = 0; i < 2L * L; i++) d[i] = (float)((double)s[i] / (double)L);
    }
    // stream-ordered behind the calls already queued: upload() synchronises the context's stream
    K.upload(k.data(), k.size(), ctx->stream);
  }
  void create(sdrhip_ctx *c, int dt, int n, const void *spectrum, int channels, size_t mb) {
    build(c, dt, n, channels, mb);
    K.alloc((size_t)L * elem());
    set_kernel(spectrum);
    tail.alloc((size_t)C * N * elem());
    tail.zero(ctx->stream);
    if (fused) {
      // enough strands that a single channel with many blocks still fills the CUs: as many as are resident at once
      const int per_cu = std::max(1, (int)((160 * 1024) / fp.lds_bytes()));
      const long want = (long)ctx->prop.multiProcessorCount * per_cu;
      max_str = (int)std::min<long>((long)max_blocks, std::max<long>(1, (want + C - 1) / C));
      stail.alloc((size_t)C * max_str * N * elem());
      if (L == 8192) allow_lds_max(fftsource_inv_kernel<512, 8>, fp.lds_bytes());
      if (L == 16384) allow_lds_max(fftsource_inv_kernel<512, 16>, fp.lds_bytes());
    }
    SDRHIP_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  }
  void launch(const void *spec, size_t nb, size_t spec_stride, void *out, size_t out_stride) {
    ctx->use();
    const long Ll = L;
    if (fused) {
      const int bps = (int)ceil_div(nb, (size_t)max_str), nstr = (int)ceil_div(nb, (size_t)bps);
      const dim3 grid((unsigned)nstr, (unsigned)C);
#define SDRHIP_SPLIT_INV(NT_, R_) hipLaunchKernelGGL((fftsource_inv_kernel<NT_, R_>), grid, dim3(NT_), fp.lds_bytes(), ctx->stream, \
    fp.dev, pos_of.p, reinterpret_cast<const float2 *>(K.p), static_cast<const float2 *>(spec), (long)spec_stride, (int)nb, bps, \
    reinterpret_cast<const float2 *>(tail.p), reinterpret_cast<float2 *>(stail.p), static_cast<float2 *>(out), (long)out_stride)
      switch (L) {
        case 2048: SDRHIP_SPLIT_INV(128, 8); break;
        case 4096: SDRHIP_SPLIT_INV(256, 8); break;
        case 8192: SDRHIP_SPLIT_INV(512, 8); break;
        default: SDRHIP_SPLIT_INV(512, 16); break;
      }
#undef SDRHIP_SPLIT_INV
      hipLaunchKernelGGL(fftsplit_fixup_kernel<float2>, dim3((unsigned)ceil_div(N, 256), (unsigned)C), dim3(256), 0, ctx->stream, N,
                         nstr, bps, reinterpret_cast<const float2 *>(stail.p), reinterpret_cast<float2 *>(tail.p),
                         static_cast<float2 *>(out), (long)out_stride);
    } else if (dtype == SDRHIP_T_CF32) {
      float2 *Y = reinterpret_cast<float2 *>(scratch.p);
      const long total = (long)C * nb * Ll;
      hipLaunchKernelGGL(fftsplit_mul_kernel<float2>, grid1d(total), dim3(256), 0, ctx->stream, static_cast<const float2 *>(spec),
                         (long)spec_stride, reinterpret_cast<const float2 *>(K.p), Ll, (long)nb * Ll, total, Y);
      exec(+1, (int)(C * nb), Y, Y);
      hipLaunchKernelGGL(fftsplit_ola_kernel<float2>, dim3((unsigned)ceil_div(N, 256), (unsigned)C), dim3(256), 0, ctx->stream, Y, N, Ll,
                         (int)nb, reinterpret_cast<float2 *>(tail.p), static_cast<float2 *>(out), (long)out_stride);
    } else {
      double2 *Y = reinterpret_cast<double2 *>(scratch.p);
      const long total = (long)C * nb * Ll;
      hipLaunchKernelGGL(fftsplit_mul_kernel<double2>, grid1d(total), dim3(256), 0, ctx->stream, static_cast<const double2 *>(spec),
                         (long)spec_stride, reinterpret_cast<const double2 *>(K.p), Ll, (long)nb * Ll, total, Y);
      exec(+1, (int)(C * nb), Y, Y);
      hipLaunchKernelGGL(fftsplit_ola_kernel<double2>, dim3((unsigned)ceil_div(N, 256), (unsigned)C), dim3(256), 0, ctx->stream, Y, N, Ll,
                         (int)nb, reinterpret_cast<double2 *>(tail.p), static_cast<double2 *>(out), (long)out_stride);
    }
    SDRHIP_CHECK_HIP(hipGetLastError());
  }
};

extern "C" {

// (FilterSink and FilterSource keep their create as it is: its messages — "out is NULL", build()'s "context is NULL" and
// bare ranges — and its codes differ from make_handle's, and *out is left alone on failure: drifted, kept)
int sdrhip_fftsink_create(sdrhip_ctx *ctx, int dtype, int N, int channels, size_t max_blocks, sdrhip_fftsink **out) {
  return guarded([&] {
    SDRHIP_REQUIRE(out, SDRHIP_E_INVALID, "out is NULL");
    std::unique_ptr<sdrhip_fftsink> h(new sdrhip_fftsink());
    h->build(ctx, dtype, N, channels, max_blocks);
    if (h->fused && h->fp.lds_bytes() > 64 * 1024) {
      if (h->nt == 512) allow_lds_max(fftsink_fwd_kernel<512>, h->fp.lds_bytes());
      else allow_lds_max(fftsink_fwd_kernel<1024>, h->fp.lds_bytes());
    }
    SDRHIP_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    *out = h.release();
  });
}

int sdrhip_fftsink_form(sdrhip_fftsink *h, const char **name) {
  return guarded([&] {
    SDRHIP_REQUIRE(h && name, SDRHIP_E_INVALID, "NULL argument");
    *name = h->form();
  });
}

// (FilterSink counts in blocks: its head is blocks_of — whole blocks, at most max_blocks — where the other nodes have max_in)
int sdrhip_fftsink_process_dev(sdrhip_fftsink *h, const void *in_dev, size_t n_in, size_t in_stride, void *spec_dev,
                               size_t spec_stride) {
  return guarded([&] {
    Range roctx_range("sdrhip_fftsink_process_dev");
    SDRHIP_REQUIRE(h, SDRHIP_E_INVALID, "handle is NULL");
    const size_t nb = h->blocks_of(n_in);
    if (nb == 0) return;
    SDRHIP_REQUIRE(in_dev && spec_dev, SDRHIP_E_INVALID, "NULL buffer");
    const size_t row = nb * (size_t)h->L;
    const Strides s = call_strides("the row", n_in, in_stride, row, spec_stride, STRIDES_TOGETHER);
    require_disjoint(in_dev, s.in, n_in, h->elem(), spec_dev, s.out, row, h->elem(), (size_t)h->C);
    h->launch(in_dev, nb, s.in, spec_dev, s.out);
  });
}

int sdrhip_fftsink_process(sdrhip_fftsink *h, const void *in_host, size_t n_in, size_t in_stride, void *spec_host,
                           size_t spec_stride) {
  return guarded([&] {
    Range roctx_range("sdrhip_fftsink_process");
    SDRHIP_REQUIRE(h, SDRHIP_E_INVALID, "handle is NULL");
    const size_t nb = h->blocks_of(n_in);
    if (nb == 0) return;
    SDRHIP_REQUIRE(in_host && spec_host, SDRHIP_E_INVALID, "NULL buffer");
    const size_t row = nb * (size_t)h->L, e = h->elem(), C = (size_t)h->C;
    const Strides s = call_strides("the row", n_in, in_stride, row, spec_stride, STRIDES_TOGETHER);
    run_staged(h->ctx, h->stage, C * h->max_blocks * h->N * e, C * h->max_blocks * h->L * e, {in_host, s.in * e, n_in * e, C},
               {spec_host, s.out * e, row * e, C}, [&](void *in, void *out) {
                 h->launch(in, nb, n_in, out, row);
                 return row * e;
               });
  });
}

int sdrhip_fftsink_destroy(sdrhip_fftsink *h) {
  return guarded([&] { destroy_handle(h); });
}

int sdrhip_fftsource_create(sdrhip_ctx *ctx, int dtype, int N, const void *kernel_spectrum, int channels, size_t max_blocks,
                            sdrhip_fftsource **out) {
  return guarded([&] {
    SDRHIP_REQUIRE(out, SDRHIP_E_INVALID, "out is NULL");
    std::unique_ptr<sdrhip_fftsource> h(new sdrhip_fftsource());
    h->create(ctx, dtype, N, kernel_spectrum, channels, max_blocks);
    *out = h.release();
  });
}

int sdrhip_fftsource_form(sdrhip_fftsource *h, const char **name) {
  return guarded([&] {
    SDRHIP_REQUIRE(h && name, SDRHIP_E_INVALID, "NULL argument");
    *name = h->form();
  });
}

int sdrhip_fftsource_set_kernel(sdrhip_fftsource *h, const void *kernel_spectrum) {
  return guarded([&] {
    SDRHIP_REQUIRE(h, SDRHIP_E_INVALID, "handle is NULL");
    h->set_kernel(kernel_spectrum);
  });
}

int sdrhip_fftsource_process_dev(sdrhip_fftsource *h, const void *spec_dev, size_t n_blocks, size_t spec_stride, void *out_dev,
                                 size_t out_stride) {
  return guarded([&] {
    Range roctx_range("sdrhip_fftsource_process_dev");
    SDRHIP_REQUIRE(h, SDRHIP_E_INVALID, "handle is NULL");
    SDRHIP_REQUIRE(n_blocks <= h->max_blocks, SDRHIP_E_SIZE, "%zu blocks > max_blocks %zu", n_blocks, h->max_blocks);
    if (n_blocks == 0) return;
    SDRHIP_REQUIRE(spec_dev && out_dev, SDRHIP_E_INVALID, "NULL buffer");
    const size_t row = n_blocks * (size_t)h->L, n = n_blocks * (size_t)h->N;
    const Strides s = call_strides("the row", row, spec_stride, n, out_stride, STRIDES_TOGETHER);
    require_disjoint(spec_dev, s.in, row, h->elem(), out_dev, s.out, n, h->elem(), (size_t)h->C);
    h->launch(spec_dev, n_blocks, s.in, out_dev, s.out);
  });
}

int sdrhip_fftsource_process(sdrhip_fftsource *h, const void *spec_host, size_t n_blocks, size_t spec_stride, void *out_host,
                             size_t out_stride) {
  return guarded([&] {
    Range roctx_range("sdrhip_fftsource_process");
    SDRHIP_REQUIRE(h, SDRHIP_E_INVALID, "handle is NULL");
    SDRHIP_REQUIRE(n_blocks <= h->max_blocks, SDRHIP_E_SIZE, "%zu blocks > max_blocks %zu", n_blocks, h->max_blocks);
    if (n_blocks == 0) return;
    SDRHIP_REQUIRE(spec_host && out_host, SDRHIP_E_INVALID, "NULL buffer");
    const size_t row = n_blocks * (size_t)h->L, n = n_blocks * (size_t)h->N, e = h->elem(), C = (size_t)h->C;
    const Strides s = call_strides("the row", row, spec_stride, n, out_stride, STRIDES_TOGETHER);
    run_staged(h->ctx, h->stage, C * h->max_blocks * h->L * e, C * h->max_blocks * h->N * e, {spec_host, s.in * e, row * e, C},
               {out_host, s.out * e, n * e, C}, [&](void *in, void *out) {
                 h->launch(in, n_blocks, row, out, n);
                 return n * e;
               });
  });
}

int sdrhip_fftsource_reset(sdrhip_fftsource *h) {
  return guarded([&] {
    use_handle(h);
    h->tail.zero(h->ctx->stream);
  });
}

int sdrhip_fftsource_destroy(sdrhip_fftsource *h) {
  return guarded([&] { destroy_handle(h); });
}

}  // extern "C"
