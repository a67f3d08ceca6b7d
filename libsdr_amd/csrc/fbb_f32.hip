// fbb_f32.hip — float baseband for BASELINE config 2 (build-defined):
//   y = SubSample_D( FIRLowPass_cf32( x[n] * exp(-2 pi i Fc n / Fs) ) )
// The reference has NO float baseband: IQBaseBand<float> does not compile (src/baseband.hh:29,205)
// and FreqShift<float> truncates samples to int16 (src/utils.hh:497-504, src/operators.hh:40-42;
// SURVEY fact 6). The reference-pinned sub-steps are the cf32 FIR (src/firfilter.hh:231-247) and
// SubSample<cf32> (src/subsample.hh:92-101), both provided by fir.hip (K3); the frequency shift is
// defined by this build: the phasor is a closed form of the absolute sample index in float64
// (oracle orc_freqshift_cf32); it is applied inside the FIR kernel's staging loop (fir.hip,
// fir_cf32_rt_kernel: closed form per lane and tile, constant float64 rotation in between), so the
// whole chain is ONE launch with 8 B read + 1 B written per input sample. PARITY UNPINNED for the shift.
#include "sdrhip_internal.hpp"
#include "entry.hpp"

using namespace sdrhip;

struct sdrhip_fbb_f32 {
  sdrhip_ctx *ctx = nullptr;
  sdrhip_fir *fir = nullptr;
  double fc = 0, fs = 1;
  int C = 1;
  size_t max_in = 0;
  unsigned long long n0 = 0;
  Staging stage;
  size_t max_out = 0;
  ~sdrhip_fbb_f32() { if (fir) sdrhip_fir_destroy(fir); }   // (create's failure path and destroy)
};

extern "C" {

int sdrhip_fbb_f32_create(sdrhip_ctx *ctx, double Fc, double Fs, const double *alpha, int order, int decim,
                          int channels, size_t max_in, sdrhip_fbb_f32 **out) {
  return guarded([&] {
    make_handle(ctx, out, alpha != nullptr, [&](sdrhip_fbb_f32 *h) {
      SDRHIP_REQUIRE(Fs > 0, SDRHIP_E_INVALID, "sample rate must be positive");
      h->fc = Fc; h->fs = Fs; h->C = channels; h->max_in = max_in;
      // (channels, max_in, order and decim are the FIR's to check)
      int rc = fir_create_impl(ctx, SDRHIP_FIR_CF32, alpha, order, decim, channels, max_in, SDRHIP_EPI_NONE, false, &h->fir);   // (the shift rides in the time-domain kernel's staging)
      if (rc != SDRHIP_OK) throw Failure{rc};
      fir_set_shift(h->fir, Fc, Fs);   // the shift rides in the FIR's staging: one kernel, no intermediate buffer
      h->max_out = max_in / decim + 1;
    });
  });
}

int sdrhip_fbb_f32_out_count(sdrhip_fbb_f32 *h, size_t n_in, size_t *n_out) {
  if (!h) { set_error("handle is NULL"); return SDRHIP_E_INVALID; }
  return sdrhip_fir_out_count(h->fir, n_in, n_out);
}

int sdrhip_fbb_f32_kernel_names(sdrhip_fbb_f32 *h, size_t n_in, char *buf, size_t len) {
  if (!h) { set_error("handle is NULL"); return SDRHIP_E_INVALID; }
  return sdrhip_fir_kernel_names(h->fir, n_in, buf, len);
}

int sdrhip_fbb_f32_last_kernels(sdrhip_fbb_f32 *h, char *buf, size_t len) {
  if (!h) { set_error("handle is NULL"); return SDRHIP_E_INVALID; }
  return sdrhip_fir_last_kernels(h->fir, buf, len);
}

int sdrhip_fbb_f32_process_dev(sdrhip_fbb_f32 *h, const float *in_dev, size_t n_in, size_t in_stride, float *out_dev,
                               size_t out_stride, size_t *n_out) {
  return guarded([&] {
    Range roctx_range("sdrhip_fbb_f32_process_dev");
    if (h) fir_clear_log(h->fir);
    if (!call_begin(h, "n_in", n_in, in_dev, out_dev)) { if (n_out) *n_out = 0; return; }
    // the strides, the overlap and the launch are the FIR's device entry point's
    int rc = sdrhip_fir_process_dev(h->fir, in_dev, n_in, in_stride, out_dev, out_stride, n_out);
    if (rc != SDRHIP_OK) throw Failure{rc};
    h->n0 += n_in;
  });
}

int sdrhip_fbb_f32_process(sdrhip_fbb_f32 *h, const float *in_host, size_t n_in, size_t in_stride, float *out_host,
                           size_t out_stride, size_t *n_out) {
  return guarded([&] {
    Range roctx_range("sdrhip_fbb_f32_process");
    if (h) fir_clear_log(h->fir);
    if (!call_begin(h, "n_in", n_in, in_host, out_host)) { if (n_out) *n_out = 0; return; }
    size_t no = 0;
    int rc = sdrhip_fir_out_count(h->fir, n_in, &no);
    if (rc != SDRHIP_OK) throw Failure{rc};
    // (no in_stride check, as the FIR's host entry point: looks like an oversight, kept)
    const Strides s = call_strides("n_in", n_in, in_stride, no, out_stride, STRIDE_OUT);
    const size_t C = (size_t)h->C;
    size_t produced = 0;
    run_staged(h->ctx, h->stage, C * h->max_in * 8, C * h->max_out * 8, {in_host, s.in * 8, n_in * 8, C},
               {out_host, s.out * 8, h->max_out * 8, C}, [&](void *in, void *out) {
                 fir_launch(h->fir, in, n_in, n_in, out, h->max_out, &produced);
                 h->n0 += n_in;
                 return produced * 8;
               });
    if (n_out) *n_out = produced;
  });
}

int sdrhip_fbb_f32_set_taps(sdrhip_fbb_f32 *h, const double *alpha) {
  return guarded([&] {
    SDRHIP_REQUIRE(h && alpha, SDRHIP_E_INVALID, "NULL argument");
    const int rc = sdrhip_fir_set_taps(h->fir, alpha);
    if (rc != SDRHIP_OK) throw Failure{rc};
  });
}

int sdrhip_fbb_f32_set_shift(sdrhip_fbb_f32 *h, double Fc) {
  return guarded([&] {
    SDRHIP_REQUIRE(h, SDRHIP_E_INVALID, "handle is NULL");
    h->fc = Fc;
    fir_set_shift(h->fir, Fc, h->fs);   // the phasor restarts at the current sample; history and decimator go on
  });
}

int sdrhip_fbb_f32_reset(sdrhip_fbb_f32 *h) {
  return guarded([&] {
    SDRHIP_REQUIRE(h, SDRHIP_E_INVALID, "handle is NULL");
    h->n0 = 0;
    int rc = sdrhip_fir_reset(h->fir);
    if (rc != SDRHIP_OK) throw Failure{rc};
  });
}

int sdrhip_fbb_f32_destroy(sdrhip_fbb_f32 *h) {
  return guarded([&] { destroy_handle(h); });   // (~sdrhip_fbb_f32 releases the FIR)
}

}  // extern "C"
