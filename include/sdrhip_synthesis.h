/* sdrhip_synthesis.h — the polyphase synthesis bank of libsdrhip.so: channel rows to ONE wideband complex row, the mirror of the
 * channelizer (sdrhip_channelizer.h). An addition to sdrhip.h, which it includes; the error codes and conventions are that
 * header's. The node has a definition of its own and no reference node behind it; its check is the numpy float64 restatement
 * tests/synthesis_restatement.py, held to <= 1e-5 of the largest output.
 *
 * What the node computes. The input is rows of complex float, channel-major: row i belongs to channel idx[i], a call brings n
 * columns (one sample per row), in_stride in complex elements — exactly the layout sdrhip_channelizer_process_dev writes.
 * Channels that are not listed carry zero. The column index m counts from 0 at create or reset, c_k[m] = 0 for m < 0. Parameters:
 *   M          the number of channels, which is also the DFT size: 2 ... 4096, prime factors in {2, 3, 5, 7, 11, 13}
 *   D          the interpolation, 1 <= D <= M. D = M is critically sampled; any other value is allowed too
 *   g[0 ... n_taps)   the prototype low-pass, given as doubles and rounded ONCE to float32 (round to nearest); the rounded values
 *              are what the node and the restatement use. 1 <= n_taps <= 64 D, so that Q = ceil(n_taps / D) <= 64.
 * The output is one row of complex float, exactly n D samples per call: the output times t in [N D, (N + n) D), N the columns
 * consumed so far,
 *
 *     z[t] = sum over k, m of  c_k[m] * g[t - m D] * exp(+2 pi i k t / M),      g[l] = 0 outside [0, n_taps)
 *
 * i.e. every channel row is interpolated by D with g and mixed up to its centre (k fs / M); the mixer's phase is zero at t = 0
 * and continuous over calls. It is the conjugate of the analysis bank's mixer: a synthesis row fed to a channelizer of the same M
 * comes back on the same channel index. The node's state is the count N and the last Q - 1 transformed columns.
 *
 * How it is computed (exact algebra, so the restatement and the kernels agree up to rounding):
 *     v_m[j] = sum over k of  c_k[m] * exp(+2 pi i k j / M)                     (an unnormalised backward DFT, float32)
 *     z[t]   = sum over q in [0, Q) with q D + d < n_taps, in that order, of  g[q D + d] * v_(m0 - q)[t mod M]
 *              with m0 = t div D, d = t mod D                                   (float32 fma chain)
 * A term with q D + d >= n_taps is skipped, not multiplied by a padded zero; the columns before the stream's start are zeros.
 * Every v and every z is computed with the same operations in the same order wherever a call or tile boundary falls and whichever
 * channels are selected, so three results hold BIT FOR BIT: the output stream does not depend on how the columns are cut into
 * calls, a selection equals the all-rows call given zero rows for the other channels, and rows and idx may be permuted together.
 *
 * The kernels, two launches per call on the context's stream:
 *   synthesis_transform_kernel   a workgroup takes a tile of T consecutive columns, T = min(256, E / M) with E = 4096 complex
 *       elements of LDS for M <= 512 and 8192 above (the channelizer's rule, images M + 1 elements apart). It reads every selected
 *       row's T contiguous samples, places each at the digit-reversed position of its channel in its column's zeroed LDS image,
 *       runs the backward decimation-in-time passes of the library's general FFT plan over all T images at once and stores every
 *       v in natural order into the handle's column workspace: a ring of Q - 1 + max_in columns of M, of which the Q - 1 columns
 *       before the write position are the state. A call's columns never land on the state's, so no block reads what another
 *       writes, and nothing is copied behind a call.
 *   synthesis_overlap_kernel     a lane per output time, lanes along t: the reads of a column are contiguous in t mod M, the taps
 *       contiguous in d; each lane sums its <= Q terms and stores z[t].
 */
#ifndef SDRHIP_SYNTHESIS_H
#define SDRHIP_SYNTHESIS_H

#include "sdrhip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sdrhip_synthesis sdrhip_synthesis;

/* taps: n_taps doubles, copied. max_in: the longest call, in columns.
 * Errors, checked in this order and BEFORE the context (host rules): NULL out / taps SDRHIP_E_INVALID; M outside [2, 4096]
 * SDRHIP_E_SIZE; M with a prime factor above 13 SDRHIP_E_INVALID; D outside [1, M] SDRHIP_E_INVALID; n_taps outside [1, 64 D]
 * SDRHIP_E_SIZE; max_in outside [1, 2^30) SDRHIP_E_SIZE; max_in D >= 2^30 SDRHIP_E_SIZE; a workspace of (Q - 1 + max_in) M above
 * 2^28 elements SDRHIP_E_SIZE; a tap that is not finite as a float SDRHIP_E_INVALID; then ctx = NULL: SDRHIP_E_NODEVICE on a
 * machine without a usable device, SDRHIP_E_INVALID elsewhere. */
int sdrhip_synthesis_create(sdrhip_ctx *ctx, int M, int D, const double *taps, int n_taps, size_t max_in, sdrhip_synthesis **out);

/* the outputs of a call of n columns: n D */
int sdrhip_synthesis_out_count(sdrhip_synthesis *h, size_t n, size_t *n_out);

/* One row per selected channel in, n columns each, in_stride in complex float elements (0 = n; below n: SDRHIP_E_SIZE); out: one
 * row of n D complex floats; *n_out (may be NULL): the outputs written. Any n up to max_in (above: SDRHIP_E_SIZE); n = 0 does
 * nothing. _process_dev: two launches on the context's stream, nothing is synchronised; the output extent must not overlap the
 * input's (SDRHIP_E_INVALID). The kernels read in[row][0 ... n) of the selected rows, nothing before or behind them. */
int sdrhip_synthesis_process_dev(sdrhip_synthesis *h, const void *in_dev, size_t n, size_t in_stride, void *out_dev, size_t *n_out);
int sdrhip_synthesis_process(sdrhip_synthesis *h, const void *in_host, size_t n, size_t in_stride, void *out_host, size_t *n_out);

/* Row i of the later calls belongs to channel idx[i]: 1 <= n_sel <= M rows, any order, every index in [0, M) and no index twice
 * (else SDRHIP_E_INVALID, nothing changes). idx = NULL: all M channels in order again. The stream itself goes on untouched. Ordered
 * on the context's stream behind the calls already enqueued. */
int sdrhip_synthesis_set_channels(sdrhip_synthesis *h, const int *idx, int n_sel);
/* a new prototype of the same length (n_taps doubles, rounded as at create; a tap that is not finite: SDRHIP_E_INVALID, nothing
 * changes); the count and the stored columns are kept. Ordered as set_channels is. */
int sdrhip_synthesis_set_taps(sdrhip_synthesis *h, const double *taps);
/* as freshly created (t = 0, stored columns of zeros), with the current taps and selection */
int sdrhip_synthesis_reset(sdrhip_synthesis *h);
/* behind the calls enqueued so far: *consumed, the columns taken since create or reset, and cols, the last Q - 1 transformed
 * columns v as [Q - 1][M] complex floats, oldest first (zeros where the stream is shorter). cols_len >= (Q - 1) M complex elements
 * where cols is given (SDRHIP_E_SIZE); either pointer may be NULL. */
int sdrhip_synthesis_get_state(sdrhip_synthesis *h, uint64_t *consumed, float *cols, size_t cols_len);
/* the geometry of a launch, any pointer may be NULL: a workgroup of the transform takes tile_times consecutive columns, an output
 * sums up to branch_taps = Q = ceil(n_taps / D) products, the workgroup's LDS images take lds_bytes, and `rows` rows are read */
int sdrhip_synthesis_plan_info(sdrhip_synthesis *h, int *tile_times, int *branch_taps, int *lds_bytes, int *rows);
/* "synthesis_transform_kernel,synthesis_overlap_kernel": the two kernels every call of the handle runs, in launch order */
int sdrhip_synthesis_kernel_names(sdrhip_synthesis *h, char *buf, size_t len);
int sdrhip_synthesis_destroy(sdrhip_synthesis *h);

#ifdef __cplusplus
}
#endif
#endif
