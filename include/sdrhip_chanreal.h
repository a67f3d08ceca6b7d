/* sdrhip_chanreal.h — the channelizer family of libsdrhip.so for a REAL-sampled antenna row (a direct-sampling HF front end, an
 * IF tap, a sound card): sdrhip_channelizer.h, sdrhip_chanaudio.h and sdrhip_chanpower.h with one row of int16 or float32 samples
 * in and the M / 2 + 1 distinct channels out, computed with a transform of half the size. An addition to those three headers,
 * which it includes; this header adds type codes and three create calls, and EVERY other call of the three headers serves the
 * handles they return (as sdrhip_tunerbb_i16_create's handles are served by the sdrhip_tuner_i16_* calls). The check is the numpy
 * float64 restatement tests/chanreal_restatement.py, held to <= 1e-5 of the largest output.
 *
 * What the nodes compute. The input is one row of real samples x[t], t counting from 0 at create or reset, x[t] = 0 for t < 0;
 * int16 is converted exactly to float. M is even, 4 ... 4096, and H = M / 2 has prime factors in {2, 3, 5, 7, 11, 13}. D, h,
 * n_taps, max_in, t_m = (m + 1) D - 1 and the output count of a call are sdrhip_channelizer.h's. The channels are k = 0 ... H,
 * K = H + 1 of them (channel M - k is the conjugate of channel k and is not produced):
 *
 *     y_k[m] = sum over l in [0, n_taps) of  h[l] * x[t_m - l] * exp(-2 pi i k (t_m - l) / M)
 *
 * — the complex node's definition applied to (x, 0). y_0 and y_H have a zero imaginary part.
 *
 * How it is computed (exact algebra). With P = ceil(n_taps / M), r in [0, M):
 *     u_m[r]  = sum over p in [0, P) with p M + r < n_taps, in that order, of  h[p M + r] * x[t_m - p M - r]
 *               (a real float32 fma chain: the complex form's with the imaginary half gone)
 *     w_m[(r - t_m) mod M] = u_m[r]
 *     z[j]    = w[2 j] + i w[2 j + 1],  j in [0, H)
 *     Z[k]    = sum over j in [0, H) of  z[j] * exp(+2 pi i k j / H)      (an unnormalised backward H-point DFT, float32: the
 *               passes of the library's general FFT plan for H points)
 *     E[k]    = (Z[k] + conj Z[(H - k) mod H]) / 2
 *     O[k]    = (Z[k] - conj Z[(H - k) mod H]) / (2 i)
 *     y_k     = E[k] + exp(+2 pi i k / M) * O[k]   for k < H,      y_H = Re E[0] - Re O[0]
 * The untangling pass, in float32 and in this order: for k in [0, H / 2], with kp = (H - k) mod H, a = Z[k], b = Z[kp] and
 * (c, s) = exp(+2 pi i k / M) — cos and sin taken in double at create and rounded once to float32 —
 *     er = 0.5 * (a.re + b.re)      ei = 0.5 * (a.im - b.im)
 *     qr = 0.5 * (a.im + b.im)      qi = 0.5 * (b.re - a.re)
 *     pr = fma(c, qr, -(s * qi))    pi = fma(c, qi, s * qr)
 *     y_k  = (er + pr, ei + pi)
 *     y_kp = (er - pr, pi - ei)     where kp != k (H even: k = H / 2 pairs with itself and only y_k is taken);
 *                                   for k = 0 this second value is y_H
 * Every output time is computed with the same operations in the same order wherever a call boundary falls, whichever channels
 * are selected and whichever of the three nodes asks, so the family's bit-for-bit properties hold for these handles too: the
 * stream does not depend on how it is cut into calls, a selected row equals that row of the all-channels run, and the three
 * nodes agree on the spectra.
 *
 * The plan. A workgroup's image of one output time holds the H + 1 channels at ld = (H + 1) | 1 complex elements (odd, so that
 * consecutive images start two LDS banks apart), and a workgroup takes T = min(256, E / M) consecutive output times with
 * E = 4096 for M <= 512 and 8192 above — the complex form's T, so a call has as many workgroups as the complex form's and each
 * takes half the LDS: T ld 8 bytes, at most 4 E + 16 T — 32 KiB + 16 bytes at M = 4096 (T = 2, ld = 2049), 32 KiB + 232 bytes at
 * the worst M (546) — so four workgroups fit a CU's 160 KiB. (Twice the tile times would fit the complex form's LDS, but halve the
 * workgroups of a call: a 2^21-sample call at M = 1024 would fill half the device and take 1.6 times as long) The
 * audio node holds one image more (its halo).
 *
 * What differs on a handle of these create calls, in the calls of the three headers:
 *   - the input element is one int16 (2 bytes) or one float (4 bytes); the overlap checks use that size;
 *   - channel indices lie in [0, H], at most K rows; set_channels(NULL) selects 0 ... H in order;
 *   - every per-channel array has K entries: modes, gains, `last`, sums, levels, flags, thresholds; get_occupied answers
 *     indices in [0, H];
 *   - get_state returns the tail as (re, 0) pairs, n_taps - 1 of them: the complex handles' layout;
 *   - kernel_names answers channelizer_real_s16_kernel / channelizer_real_f32_kernel, chanaudio_real_s16_kernel / chanaudio_real_f32_kernel,
 *     chanpower_real_s16_kernel / chanpower_real_f32_kernel (the last two followed by ",chanpower_finish_kernel");
 *   - plan_info reports this plan's tile times, LDS bytes and rows; branch_taps is ceil(n_taps / M) as before.
 */
#ifndef SDRHIP_CHANREAL_H
#define SDRHIP_CHANREAL_H

#include "sdrhip_channelizer.h"
#include "sdrhip_chanaudio.h"
#include "sdrhip_chanpower.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the input's element type at the three create calls below */
enum { SDRHIP_CHANREAL_S16 = 0, SDRHIP_CHANREAL_F32 = 1 };

/* The names: the exports beginning sdrhip_channelizer, sdrhip_chanaudio and sdrhip_chanpower are exactly their headers' lists
 * (the ABI tests of the three headers hold the library to that), so these three begin sdrhip_chanreal; for the same reason the
 * kernels are *_real_s16_kernel and *_real_f32_kernel.
 * As sdrhip_channelizer_create, sdrhip_chanaudio_create (modes and gains: K = M / 2 + 1 entries each, or NULL) and
 * sdrhip_chanpower_create. Errors, checked in the order of those calls and BEFORE the context (host rules): NULL out / taps
 * SDRHIP_E_INVALID; dtype SDRHIP_E_INVALID; M outside [4, 4096] SDRHIP_E_SIZE; M odd, or M / 2 with a prime factor above 13,
 * SDRHIP_E_INVALID; then D, n_taps, max_in, the taps and the node's own arguments as in those calls; then ctx. */
int sdrhip_chanreal_channelizer_create(sdrhip_ctx *ctx, int dtype, int M, int D, const double *taps, int n_taps, size_t max_in,
                                       sdrhip_channelizer **out);
int sdrhip_chanreal_audio_create(sdrhip_ctx *ctx, int dtype, int M, int D, const double *taps, int n_taps, size_t max_in,
                                 const int *modes, const float *gains, sdrhip_chanaudio **out);
int sdrhip_chanreal_power_create(sdrhip_ctx *ctx, int dtype, int M, int D, const double *taps, int n_taps, size_t max_in, double alpha,
                                 sdrhip_chanpower **out);

#ifdef __cplusplus
}
#endif
#endif
