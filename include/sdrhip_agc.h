/* sdrhip_agc.h — the AGC bank of libsdrhip.so: the reference's AGC<int16_t> / AGC<float> (src/utils.hh:658-793), one node per
 * row, all rows in one launch. An addition to sdrhip.h, which it includes; the error codes and conventions are that header's.
 *
 * What a node computes, in IEEE float32 with every operation rounded on its own (no fused multiply-add), per sample x:
 *     a    = float(|x|)                     int16: |x| as int, so |-32768| = 32768
 *     sd   = lambda * sd + (1 - lambda) * a   (1 - lambda) is one float, computed once
 *     gain = target / (4 * sd)              only while enabled; correctly rounded, denormals kept, may be +inf
 *     y    = gain * float(x)
 *     float: out = y (inf * 0 leaves a NaN)     int16: out = 0 unless |y| < 2^31, else the low 16 bits of int32(trunc(y))
 * A row that is disabled AND has gain 0 copies its samples and leaves its state alone (the reference forwards the buffer);
 * a disabled row with any other gain still updates sd and applies the held gain.
 * Fresh state of a row: sd = target, gain = 1, enabled.
 *
 * Deviation from the reference: AGC::process sends its whole output buffer whatever the input's length; this node writes the
 * n samples of the call and nothing behind them.
 */
#ifndef SDRHIP_AGC_H
#define SDRHIP_AGC_H

#include "sdrhip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { SDRHIP_AGC_I16 = 0, SDRHIP_AGC_F32 = 1 };

typedef struct sdrhip_agc sdrhip_agc;

/* Designers (host only). lambda = float(exp(-1 / (double(float(tau)) * sample_rate))): the reference keeps tau in a float
 * member and narrows the double exp once. SDRHIP_E_INVALID: NULL, tau or sample_rate not above 0. */
int sdrhip_design_agc_lambda(double tau, double sample_rate, float *lambda);
/* the target the reference picks for AGC(tau, 0): 16000 for int16, 0.5 for float */
int sdrhip_design_agc_target(int dtype, float *target);

/* `channels` rows with the same lambda and target, all enabled (sdrhip_agc_create), or with one lambda, target and enabled flag
 * per row (sdrhip_agcbank_create). Parameters and state are per row in both; the handles differ in nothing else.
 * Errors, checked in this order and BEFORE the context (host rules): NULL out / lambda / target / enabled SDRHIP_E_INVALID;
 * dtype SDRHIP_E_INVALID; channels outside 1 ... 65535 SDRHIP_E_INVALID; max_in outside [1, 2^30) SDRHIP_E_SIZE; a lambda
 * outside [0, 1) SDRHIP_E_INVALID; a target that is not finite or not above 0 SDRHIP_E_INVALID; then ctx = NULL:
 * SDRHIP_E_NODEVICE on a machine without a usable device, SDRHIP_E_INVALID elsewhere. */
int sdrhip_agc_create(sdrhip_ctx *ctx, int dtype, float lambda, float target, int channels, size_t max_in, sdrhip_agc **out);
int sdrhip_agcbank_create(sdrhip_ctx *ctx, int dtype, const float *lambda, const float *target, const int *enabled, int channels,
                          size_t max_in, sdrhip_agc **out);

/* channels rows of n samples (int16 or float, by the handle's dtype) in, as many out; strides in samples, 0 = n. Any n up to
 * max_in (above: SDRHIP_E_SIZE); n = 0 does nothing. _process_dev: one launch on the context's stream, nothing is synchronised;
 * out_dev == in_dev with equal strides works in place, any other overlap of the two extents is SDRHIP_E_INVALID. */
int sdrhip_agc_process_dev(sdrhip_agc *h, const void *in_dev, size_t n, size_t in_stride, void *out_dev, size_t out_stride);
int sdrhip_agc_process(sdrhip_agc *h, const void *in_host, size_t n, size_t in_stride, void *out_host, size_t out_stride);

/* Control calls: each is ordered on the context's stream behind the calls already enqueued, touches row c alone, and changes
 * nothing where it is refused (a row outside the bank, a lambda or target create would refuse: SDRHIP_E_INVALID).
 * _set_channel: a fresh node behind row c (sd = target, gain = 1, enabled). _set_lambda: setTau of the reference, the state
 * goes on. _set_enabled / _set_gain: enable() / setGain(); a gain that is not finite is taken as it is. */
int sdrhip_agc_set_channel(sdrhip_agc *h, int channel, float lambda, float target);
int sdrhip_agc_set_lambda(sdrhip_agc *h, int channel, float lambda);
int sdrhip_agc_set_enabled(sdrhip_agc *h, int channel, int enabled);
int sdrhip_agc_set_gain(sdrhip_agc *h, int channel, float gain);
/* gain, sd, enabled of every row after the calls enqueued so far; n >= channels (SDRHIP_E_SIZE), any pointer may be NULL.
 * sd of an AM or USB row is the running mean of |audio|: the row's signal level. */
int sdrhip_agc_get_state(sdrhip_agc *h, float *gain, float *sd, int *enabled, int n);
/* the geometry a call of n samples launches with: a workgroup takes channels_per_group rows, tile_samples samples at a time */
int sdrhip_agc_plan_info(sdrhip_agc *h, size_t n, int *tile_samples, int *channels_per_group);
int sdrhip_agc_kernel_names(sdrhip_agc *h, char *buf, size_t len);   /* "agc_i16_kernel" or "agc_f32_kernel" */
/* every row as freshly created (sd = target, gain = 1) with its current lambda, target and enabled flag */
int sdrhip_agc_reset(sdrhip_agc *h);
int sdrhip_agc_destroy(sdrhip_agc *h);

#ifdef __cplusplus
}
#endif
#endif
