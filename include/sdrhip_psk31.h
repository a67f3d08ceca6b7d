/* sdrhip_psk31.h — the BPSK31 bank of libsdrhip.so: the reference's BPSK31<int16_t> / BPSK31<float> demodulator
 * (src/psk31.hh:16-291), one node per row, all rows in one launch: complex baseband rows in, the 31.25 baud bit stream of
 * every row out. An addition to sdrhip.h, which it includes; the error codes and conventions are that header's.
 *
 * What a node computes. All arithmetic is IEEE float32, every operation rounded on its own (no fused multiply-add), denormals
 * kept; the places marked (double) are the exceptions.
 *   state of a row   P, F, mu, omega; the 8 last rotated samples (the line, oldest first); p0, p1, p2 (complex) and c0, c1, c2;
 *                    hist[64], hist_idx, last
 *   constants        Fmin = float(-dF), Fmax = float(dF); alpha = float(4 d w / t), beta = float(4 w w / t) with the doubles
 *                    d = sqrt(2) / 2, w = pi / 100, t = 1 + 2 d w + w w; omega0 = float(sample_rate / 2000.0);
 *                    min_omega = float(double(omega0) * (1.0 - double(0.001f))), max_omega = float(double(omega0) * (1.0 + double(0.001f)))
 *   a fresh row      P = F = 0, mu = 0.25, omega = omega0, last = 1, everything else 0
 * Per call, while input is left:
 *   fill, if mu > 1:   mu -= 1; P += F; wrap(P); (s, c) = psk_sincos(P); push (c * xr - s * xi, c * xi + s * xr) into the line
 *                      (four products, two sums; an int16 sample converts exactly) and consume the sample
 *   else sub-sample:   row = int(roundf(mu * 128)); out = sum over k = 0 ... 7 of line[k] * table[row][k], from 0 in tap order,
 *                      real and imaginary parts apart; with re, im = out:
 *     timing   p2 = p1, p1 = p0, p0 = out; c2 = c1, c1 = c0, c0 = re > 0 ? -1 : 1
 *              err = (p0.re - p2.re) * c1 - (c0 - c2) * p1.re, clamped to [-1, 1]
 *              omega += 0.001f * err, then max(min_omega, min(max_omega, omega)); mu += omega + 0.01f * err (this association)
 *     carrier  phi = 0 if re * re + im * im == 0, else ((-re) * im) / (re * re + im * im), the division correctly rounded
 *              F += beta * phi; P += F + alpha * phi; wrap(P); F = min(Fmax, max(Fmin, F))
 *     symbol   hist[hist_idx] = re; a transition (hist_idx > 1 and hist[hist_idx - 1] >= 0 >= re or <= 0 <= re) restarts the
 *              history (hist_idx = 0) and, if hist_idx >= 32, emits a bit before; without one a bit is emitted at hist_idx == 63,
 *              and hist_idx counts on otherwise. A bit is last == sgn with sgn = (hist[0] + ... + hist[hist_idx] > 0 ? 1 : -1),
 *              summed in float from 0 in index order; then last = sgn.
 *   wrap(P): while P > 2 pi: P = float(double(P) - 2 pi); while P < -2 pi: P = float(double(P) + 2 pi) (double); since |F| <= pi
 *            one trip is enough, the node makes at most two.
 *   min / max are std::min / std::max: a NaN omega becomes max_omega, a NaN F becomes Fmin.
 * A sub-sample that is due when a call ends is taken at the start of the next: the stream does not depend on the call lengths.
 *
 * The interpolation table (129 rows of 8 taps, row = round(128 mu)) is an ARGUMENT of create. The reference's own table has 128
 * initialisers for its 129 rows (the mirror of row 63 is missing: rows 65 ... 127 sit one place early, row 128 is all zeros, and a
 * sub-sample at mu > 0.996 is exactly 0); bit parity with the reference needs that data as it is, passed by the caller.
 * sdrhip_design_inpol_taps designs a table of this library's own, with all 129 rows.
 *
 * Deviations from the reference:
 *  1. psk_sincos. The reference's std::exp(complex<float>(0, P)) ends in the C library's sincosf, which differs between C
 *     libraries and from the correctly rounded values. The node uses a DEFINED sequence of IEEE double operations, each rounded
 *     on its own, with x = double(P):
 *         k = rint(x * (2 / pi));  r = x - k * (pi / 2);  z = r * r
 *         sr = r + (r * z) * S(z),  S = Horner in z over -1/3!, 1/5!, ... , 1/13!
 *         cr = 1 + z * C(z),        C = Horner in z over -1/2!, 1/4!, ... , -1/14!
 *         k mod 4 = 0: (sr, cr); 1: (cr, -sr); 2: (-sr, -cr); 3: (-cr, sr); then s and c are narrowed to float once.
 *     Both are within 1 ulp of float(sin(double(P))), float(cos(double(P))) on [-2 pi, 2 pi]. On the fixtures the bits are those
 *     of the reference; the state differs from it in the last digits.
 *  2. BPSK31::config sizes its output buffer for one second of input and a longer call overruns it; this node has no such limit.
 *  3. A NaN mu (from non-finite float samples only) makes the reference loop for ever; this node consumes the rest of the call.
 */
#ifndef SDRHIP_PSK31_H
#define SDRHIP_PSK31_H

#include "sdrhip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { SDRHIP_PSK31_CS16 = 0, SDRHIP_PSK31_CF32 = 1 };

typedef struct sdrhip_psk31 sdrhip_psk31;

/* Designer (host only): out[129 * 8], row r the 8-tap fractional-delay filter for mu = r / 128. Tap k weighs the line's sample at
 * time k - 4 and the row interpolates at time -mu, so row 0 is the unit impulse at tap 4 and row 128 the one at tap 3. A row is
 * the least-squares fit of sum_k h[k] e^{j w (k - 4)} to e^{-j w mu} over the band |w| <= pi / 2 (a quarter of the sample rate
 * on either side): the 8 x 8 normal equations A h = b with A[k][l] = s(k - l), b[k] = s(k - 4 + mu), s(t) = sin(pi t / 2) / (pi t)
 * and s(0) = 1 / 2, solved in double by Gaussian elimination with partial pivoting and narrowed to float. Rows 0 ... 64 are
 * solved (row 0 set to the impulse, row 64 made symmetric by averaging h[k] and h[7 - k]); rows 65 ... 128 are the mirrors of rows
 * 63 ... 0, so row r mirrors row 128 - r exactly. SDRHIP_E_INVALID: NULL. */
int sdrhip_design_inpol_taps(float *out);

/* `channels` rows at one sample rate with the same dF (sdrhip_psk31_create) or a dF per row (sdrhip_psk31bank_create); dF is the
 * range of the carrier loop in radians per sample (the reference's default: 0.1). table: 129 * 8 floats, copied.
 * Errors, checked in this order and BEFORE the context (host rules): NULL out / table / dF SDRHIP_E_INVALID; dtype
 * SDRHIP_E_INVALID; channels outside 1 ... 65535 SDRHIP_E_INVALID; max_in outside [1, 2^30) SDRHIP_E_SIZE; a sample_rate that is
 * not finite or below 2000 SDRHIP_E_INVALID; a dF outside (0, pi] SDRHIP_E_INVALID; a table entry that is not finite
 * SDRHIP_E_INVALID; then ctx = NULL: SDRHIP_E_NODEVICE on a machine without a usable device, SDRHIP_E_INVALID elsewhere. */
int sdrhip_psk31_create(sdrhip_ctx *ctx, int dtype, double sample_rate, double dF, const float *table, int channels, size_t max_in,
                        sdrhip_psk31 **out);
int sdrhip_psk31bank_create(sdrhip_ctx *ctx, int dtype, double sample_rate, const float *dF, const float *table, int channels,
                            size_t max_in, sdrhip_psk31 **out);

/* The most bits a row can write in a call of n samples; 0 for n = 0, else 1 + S / 33 with
 *     S = floor((n + 3 + max_omega) / (min_omega - 0.0100001)) + 1.
 * Why: a sub-sample is taken with 0 <= mu <= 1 and advances mu by at least min_omega - 0.01, a consumed sample takes 1 off, and mu
 * ends a call at most 1 + max_omega + 0.01; so S bounds the sub-samples of the call. A bit needs hist_idx >= 32, that is 33
 * sub-samples since the one before it; only the call's first bit can come sooner, from the history the call inherits. */
int sdrhip_psk31_out_capacity(sdrhip_psk31 *h, size_t n, size_t *bits);

/* channels rows of n complex samples (int16 or float pairs, by the handle's dtype) in, in_stride in complex samples (0 = n);
 * out: one byte (0 / 1) per bit, channels rows of out_stride bytes (0 = the capacity of n; below it: SDRHIP_E_SIZE), and
 * counts[channels] uint32: the bits row c wrote. Bytes of a row behind its count are left alone by _process_dev; _process
 * delivers them as zeros. Any n up to max_in (above: SDRHIP_E_SIZE); n = 0 writes zero counts (_process) or nothing
 * (_process_dev). _process_dev: one launch on the context's stream, nothing is synchronised. */
int sdrhip_psk31_process_dev(sdrhip_psk31 *h, const void *in_dev, size_t n, size_t in_stride, uint8_t *bits_dev, size_t out_stride,
                             uint32_t *counts_dev);
int sdrhip_psk31_process(sdrhip_psk31 *h, const void *in_host, size_t n, size_t in_stride, uint8_t *bits_host, size_t out_stride,
                         uint32_t *counts_host);

/* A fresh node with range dF behind row `channel`, ordered on the context's stream behind the calls already enqueued; the other
 * rows stream on. A row outside the bank or a dF create would refuse: SDRHIP_E_INVALID, nothing changes. */
int sdrhip_psk31_set_channel(sdrhip_psk31 *h, int channel, double dF);
/* every row as freshly created, with its current dF */
int sdrhip_psk31_reset(sdrhip_psk31 *h);
/* P, F, mu, omega, hist_idx, last of every row behind the calls enqueued so far; n >= channels (SDRHIP_E_SIZE), any pointer may
 * be NULL. */
int sdrhip_psk31_get_state(sdrhip_psk31 *h, float *P, float *F, float *mu, float *omega, int *hist_idx, int *last, int n);
/* the geometry of a launch: a workgroup takes channels_per_group rows (one wave each), tile_samples samples at a time */
int sdrhip_psk31_plan_info(sdrhip_psk31 *h, size_t n, int *tile_samples, int *channels_per_group);
int sdrhip_psk31_kernel_names(sdrhip_psk31 *h, char *buf, size_t len);   /* "psk31_cs16_kernel" or "psk31_cf32_kernel" */
int sdrhip_psk31_destroy(sdrhip_psk31 *h);

#ifdef __cplusplus
}
#endif
#endif
