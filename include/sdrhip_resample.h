/* sdrhip_resample.h — the interpolating resampler bank of libsdrhip.so: the reference's InpolSubSampler<iScalar, oScalar>
 * (src/subsample.hh:194-288, src/interpolate.hh), one node per row, all rows in one launch: rows at one sample rate in, each row
 * at its own rate (input rate / frac) out. An addition to sdrhip.h, which it includes; the error codes and conventions are that
 * header's.
 *
 * What a node computes. All arithmetic is IEEE float32, every operation rounded on its own (no fused multiply-add), denormals
 * kept.
 *   state of a row   frac (float), mu (float), the 8 last samples (the line, oldest first) in the OUTPUT type
 *   a fresh row      mu = 0, a line of zeros
 * Per call of n samples x[0 ... n), the reference's loop kept exactly:
 *     i = 0; o = 0
 *     while i < n:
 *         while mu >= 1 and i < n:   push x[i] into the line; i += 1; mu = fl(mu - 1)
 *         while mu <= 1:             out[o] = interp(line, mu); o += 1; mu = fl(mu + frac)
 *   interp(line, mu): row = int(roundf(mu * 128)); the sum over k = 0 ... 7 of line[k] * table[row][k], from 0 in tap order.
 *     float, complex float (real and imaginary parts summed apart):   acc = fl(acc + fl(line[k] * t[k]))
 *     int16: the accumulator is an int16 converted back AFTER EVERY TAP:  acc = int16(fl(float(acc) + fl(float(line[k]) * t[k]))),
 *            the conversion being the x86 one (truncate to int32, keep the low 16 bits; 0 where |value| >= 2^31): it WRAPS and
 *            does not saturate — a full-scale step at frac = 1.5 gives ... 32767 -32558 32767 ... where the float node gives 1.00649.
 *     A complex int16 sample converts exactly to complex float on entering the line (SDRHIP_RESAMPLE_CS16_CF32).
 * What follows from the loop, and is kept:
 *   - a fresh row's first call emits one output from the zero line (mu = 0) before it consumes a sample;
 *   - n = 0 emits nothing and changes nothing;
 *   - mu == 1 is taken by the first loop where input is left and by the second where not: with frac = 0.5 every second output is
 *     taken at mu == 1 (table row 128); with frac = 2 a call of odd length ends on mu == 1 with no input left and emits an output
 *     at row 128, where an unsplit stream would have pushed a sample and taken row 0. THE NODE FOLLOWS THE REFERENCE CALL BY
 *     CALL, so in this one case the stream depends on the call lengths: row 128 at window position p is not what row 0 at p + 1
 *     gives. With the reference's own table row 128 is all zeros and the output is 0; with sdrhip_design_inpol_taps row 128 is
 *     the impulse at tap 3, the sample two before the one row 0 would take at p + 1 (the tables run towards the OLDER sample as
 *     mu grows).
 *
 * The interpolation table (129 rows of 8 taps) is an ARGUMENT of create, copied — see sdrhip_psk31.h: the reference's own table,
 * quirks included, for bit parity with it; sdrhip_design_inpol_taps for a table of this library's own.
 *
 * Deviations from the reference:
 *  1. frac must be finite and lie in [0.125, 4096]. The reference takes any frac > 0 (its documentation warns against factors
 *     beyond 8).
 *  2. A row with frac == 1 is the reference's short cut: the call's n samples are copied and the state is left alone. For
 *     SDRHIP_RESAMPLE_CS16_CF32 the copy is converted; the reference would hand its int16 buffer to a float sink.
 *  3. The reference sizes its output buffer as ceil(bufferSize * sampleRate / frac) — multiplied by the sample rate: far too large
 *     at real rates and too small at a sample rate near 1, where a call overruns it. This node's output limit is the capacity:
 *
 * Capacity. sdrhip_resample_out_capacity reports the most outputs ANY row can write in a call of n: 0 for n = 0; n for a row with
 * frac == 1; else floor((n + 1) / frac) + 2, computed in double from the float frac (the bank: the largest over its rows).
 * Why: an output is taken with mu <= 1 and adds frac; a consumed sample takes 1 off and mu never goes below 0; mu ends a call at
 * most at 1 + frac. So outputs * frac <= n + 1 + frac, and the second + 1 covers the roundings of the float chain.
 */
#ifndef SDRHIP_RESAMPLE_H
#define SDRHIP_RESAMPLE_H

#include "sdrhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* input -> output element: float -> float; complex float -> complex float; int16 -> int16; complex int16 -> complex float */
enum { SDRHIP_RESAMPLE_F32 = 0, SDRHIP_RESAMPLE_CF32 = 1, SDRHIP_RESAMPLE_I16 = 2, SDRHIP_RESAMPLE_CS16_CF32 = 3 };

typedef struct sdrhip_resample sdrhip_resample;

/* `channels` rows with the same frac (sdrhip_resample_create) or a frac per row (sdrhip_resamplebank_create); the handles differ in
 * nothing else. table: 129 * 8 floats, copied.
 * Errors, checked in this order and BEFORE the context (host rules): NULL out / table / frac SDRHIP_E_INVALID; dtype
 * SDRHIP_E_INVALID; channels outside 1 ... 65535 SDRHIP_E_INVALID; max_in outside [1, 2^30) SDRHIP_E_SIZE; a frac that is not finite
 * or outside [0.125, 4096] SDRHIP_E_INVALID; a table entry that is not finite SDRHIP_E_INVALID; then ctx = NULL: SDRHIP_E_NODEVICE
 * on a machine without a usable device, SDRHIP_E_INVALID elsewhere. */
int sdrhip_resample_create(sdrhip_ctx *ctx, int dtype, float frac, const float *table, int channels, size_t max_in, sdrhip_resample **out);
int sdrhip_resamplebank_create(sdrhip_ctx *ctx, int dtype, const float *frac, const float *table, int channels, size_t max_in,
                               sdrhip_resample **out);

/* the most outputs a row can write in a call of n samples (above) */
int sdrhip_resample_out_capacity(sdrhip_resample *h, size_t n, size_t *outputs);

/* channels rows of n input elements in, in_stride in input elements (0 = n); out: channels rows of out_stride OUTPUT elements
 * (0 = the capacity of n; below it: SDRHIP_E_SIZE), and counts[channels] uint32: the outputs row c wrote. Elements of a row behind
 * its count are left alone by _process_dev; _process delivers them as zeros. Any n up to max_in (above: SDRHIP_E_SIZE); n = 0 writes
 * zero counts (_process) or nothing (_process_dev). _process_dev: one launch on the context's stream, nothing is synchronised; the
 * output extent must not overlap the input's (SDRHIP_E_INVALID). */
int sdrhip_resample_process_dev(sdrhip_resample *h, const void *in_dev, size_t n, size_t in_stride, void *out_dev, size_t out_stride,
                                uint32_t *counts_dev);
int sdrhip_resample_process(sdrhip_resample *h, const void *in_host, size_t n, size_t in_stride, void *out_host, size_t out_stride,
                            uint32_t *counts_host);

/* A fresh node with this frac behind row `channel`, ordered on the context's stream behind the calls already enqueued; the other
 * rows stream on. A row outside the bank or a frac create would refuse: SDRHIP_E_INVALID, nothing changes. */
int sdrhip_resample_set_channel(sdrhip_resample *h, int channel, float frac);
/* every row as freshly created, with its current frac */
int sdrhip_resample_reset(sdrhip_resample *h);
/* frac and mu of every row, and its line as 8 x components values (components: 2 for the complex types), oldest first: float for
 * the types with a float output (line_i16 is not written), int16 for SDRHIP_RESAMPLE_I16 (line_f32 is not written) — behind the
 * calls enqueued so far; n >= channels (SDRHIP_E_SIZE), any pointer may be NULL. */
int sdrhip_resample_get_state(sdrhip_resample *h, float *frac, float *mu, float *line_f32, int16_t *line_i16, int n);
/* the geometry of a launch: a workgroup takes channels_per_group rows, tile_samples input samples at a time */
int sdrhip_resample_plan_info(sdrhip_resample *h, size_t n, int *tile_samples, int *channels_per_group);
/* "resample_f32_kernel", "resample_cf32_kernel", "resample_i16_kernel" or "resample_cs16_cf32_kernel" */
int sdrhip_resample_kernel_names(sdrhip_resample *h, char *buf, size_t len);
int sdrhip_resample_destroy(sdrhip_resample *h);

#ifdef __cplusplus
}
#endif
#endif
