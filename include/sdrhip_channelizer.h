/* sdrhip_channelizer.h — the polyphase channelizer of libsdrhip.so: ONE antenna row to M uniform channels, each 1 / M of the band
 * wide and decimated by D, in one pass. An addition to sdrhip.h, which it includes; the error codes and conventions are that
 * header's. The node has a definition of its own and no reference node behind it (as the float baseband of config 2); its check is
 * the numpy float64 restatement tests/channelizer_restatement.py, held to <= 1e-5 of the largest output.
 *
 * What the node computes. The input is one row of complex samples x[t]; t counts from 0 at create or reset, x[t] = 0 for t < 0.
 * The element type is complex<int16> (converted exactly to float) or complex<float>. Parameters:
 *   M          the number of channels, which is also the DFT size: 2 ... 4096, prime factors in {2, 3, 5, 7, 11, 13}
 *   D          the decimation, 1 <= D <= M. D = M is critically sampled, D = M / 2 the usual 2x oversampled bank; any other value
 *              is allowed too (the identity below needs no divisibility)
 *   h[0 ... n_taps)   the prototype low-pass, given as doubles and rounded ONCE to float32 (round to nearest); the rounded values
 *              are what the node and the restatement use. 1 <= n_taps <= 64 M.
 * For channel k and output index m, with t_m = (m + 1) D - 1:
 *
 *     y_k[m] = sum over l in [0, n_taps) of  h[l] * x[t_m - l] * exp(-2 pi i k (t_m - l) / M)
 *
 * i.e. channel k's centre (k fs / M) is mixed down to 0 with the mixer's phase zero at t = 0 and continuous over calls, the result
 * is filtered with h, and the sample at the end of every block of D inputs is kept. Output is complex float. A call of n samples
 * behind N consumed ones emits floor((N + n) / D) - floor(N / D) outputs per channel; n = 0 and n < D are legal. The node's state
 * is the count N and the last n_taps - 1 samples (the tail; the samples not yet followed by an output are among them or, where
 * D > n_taps, are not needed by any later output).
 *
 * How it is computed (exact algebra, so the restatement and the kernel agree up to rounding). With P = ceil(n_taps / M) and r in
 * [0, M):
 *     u_m[r]  = sum over p in [0, P) with p M + r < n_taps, in that order, of  h[p M + r] * x[t_m - p M - r]   (float32 fma chain)
 *     w_m[(r - t_m) mod M] = u_m[r]                              (a circular shift by the absolute time, no multiply)
 *     y_k[m]  = sum over j in [0, M) of  w_m[j] * exp(+2 pi i k j / M)                 (an unnormalised backward DFT, float32)
 * Every output time is computed with the same operations in the same order wherever a call boundary falls and whichever channels
 * are selected, so two results hold BIT FOR BIT: the output stream does not depend on how the input stream is cut into calls, and
 * a selected row equals the corresponding row of the all-channels run.
 *
 * Output layout: channel-major rows. Row i holds channel sel[i], out_stride in complex elements — the rows drop into the
 * process_dev of the banks that take complex float rows (the resampler bank, the BPSK31 bank, the AGC bank). By default every
 * channel is written, in order; sdrhip_channelizer_set_channels keeps a subset (the stores are the node's memory traffic).
 *
 * The kernel (channelizer_cs16_kernel / channelizer_cf32_kernel, one form for every M): a workgroup takes a tile of T consecutive
 * output times, T = min(256, E / M) with E = 4096 complex elements of LDS for M <= 512 and 8192 above. It forms the T vectors u
 * from global reads (the input row and the taps are small and cache-resident, both contiguous in r), writes each at its shifted
 * and digit-reversed position into its LDS image, runs the backward decimation-in-time passes over all T images at once (the
 * butterflies and roots of the library's general FFT plan, so the spectra come out in natural order), and stores the spectra
 * transposed: every selected row gets T contiguous complex floats.
 */
#ifndef SDRHIP_CHANNELIZER_H
#define SDRHIP_CHANNELIZER_H

#include "sdrhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the input's element type; the output is complex float for both */
enum { SDRHIP_CHAN_CS16 = 0, SDRHIP_CHAN_CF32 = 1 };

typedef struct sdrhip_channelizer sdrhip_channelizer;

/* taps: n_taps doubles, copied. max_in: the longest call, in samples.
 * Errors, checked in this order and BEFORE the context (host rules): NULL out / taps SDRHIP_E_INVALID; dtype SDRHIP_E_INVALID;
 * M outside [2, 4096] SDRHIP_E_SIZE; M with a prime factor above 13 SDRHIP_E_INVALID; D outside [1, M] SDRHIP_E_INVALID; n_taps
 * outside [1, 64 M] SDRHIP_E_SIZE; max_in outside [1, 2^30) SDRHIP_E_SIZE; a tap that is not finite as a float SDRHIP_E_INVALID;
 * then ctx = NULL: SDRHIP_E_NODEVICE on a machine without a usable device, SDRHIP_E_INVALID elsewhere. */
int sdrhip_channelizer_create(sdrhip_ctx *ctx, int dtype, int M, int D, const double *taps, int n_taps, size_t max_in,
                              sdrhip_channelizer **out);

/* the outputs per channel of a call of n samples made NOW: floor((N + n) / D) - floor(N / D), N the samples consumed so far */
int sdrhip_channelizer_out_count(sdrhip_channelizer *h, size_t n, size_t *n_out);

/* One row of n input elements in; out: one row per selected channel, out_stride in complex float elements (0 = the call's output
 * count; below it: SDRHIP_E_SIZE); *n_out (may be NULL): the outputs written per row. Any n up to max_in (above: SDRHIP_E_SIZE);
 * n = 0 does nothing. _process_dev: one launch on the context's stream, nothing is synchronised; the output extent must not overlap
 * the input's (SDRHIP_E_INVALID). The kernel reads in[0 ... n) and the stored tail, nothing before or behind them. */
int sdrhip_channelizer_process_dev(sdrhip_channelizer *h, const void *in_dev, size_t n, void *out_dev, size_t out_stride, size_t *n_out);
int sdrhip_channelizer_process(sdrhip_channelizer *h, const void *in_host, size_t n, void *out_host, size_t out_stride, size_t *n_out);

/* Row i of the later calls holds channel idx[i]: 1 <= n_sel <= M rows, any order, every index in [0, M) and no index twice
 * (else SDRHIP_E_INVALID, nothing changes). idx = NULL: all M channels in order again. The stream itself goes on untouched. Ordered
 * on the context's stream behind the calls already enqueued. */
int sdrhip_channelizer_set_channels(sdrhip_channelizer *h, const int *idx, int n_sel);
/* a new prototype of the same length (n_taps doubles, rounded as at create; a tap that is not finite: SDRHIP_E_INVALID, nothing
 * changes); the count and the tail are kept. Ordered as set_channels is. */
int sdrhip_channelizer_set_taps(sdrhip_channelizer *h, const double *taps);
/* as freshly created (t = 0, a tail of zeros), with the current taps and selection */
int sdrhip_channelizer_reset(sdrhip_channelizer *h);
/* behind the calls enqueued so far: *consumed, the samples taken since create or reset, and tail, the last n_taps - 1 samples as
 * complex floats, oldest first (zeros where the stream is shorter). tail_len >= n_taps - 1 complex elements where tail is given
 * (SDRHIP_E_SIZE); either pointer may be NULL. */
int sdrhip_channelizer_get_state(sdrhip_channelizer *h, uint64_t *consumed, float *tail, size_t tail_len);
/* the geometry of a launch, any pointer may be NULL: a workgroup takes tile_times consecutive output times, every branch sums
 * branch_taps = ceil(n_taps / M) products, the workgroup's LDS images take lds_bytes, and `rows` rows are written */
int sdrhip_channelizer_plan_info(sdrhip_channelizer *h, int *tile_times, int *branch_taps, int *lds_bytes, int *rows);
/* "channelizer_cs16_kernel" or "channelizer_cf32_kernel": the one kernel every call of the handle runs */
int sdrhip_channelizer_kernel_names(sdrhip_channelizer *h, char *buf, size_t len);
int sdrhip_channelizer_destroy(sdrhip_channelizer *h);

#ifdef __cplusplus
}
#endif
#endif
