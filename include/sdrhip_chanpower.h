/* sdrhip_chanpower.h — the channel power monitor of libsdrhip.so: ONE antenna row to M per-channel powers, a smoothed level per
 * channel and an open / closed flag per channel with hysteresis (a squelch), on the uniform grid of sdrhip_channelizer.h. An
 * addition to sdrhip.h and sdrhip_channelizer.h, which it includes; the error codes, the dtype codes and the conventions are
 * theirs. The node is the library's own, as the channelizer is: no reference node stands behind it, its definition is written
 * here and its check is the numpy float64 restatement tests/chanpower_restatement.py. It answers the question the channelizers'
 * set_channels asks — which channels carry something — without a row leaving the device or being stored on it.
 *
 * The stream is the channelizer's. With M, D, h[0 ... n_taps) as in sdrhip_channelizer.h, y_k[m] is exactly the value
 * sdrhip_channelizer computes, for all M channels always (the monitor has no row selection): the float32 re, im of an output
 * are bit for bit the plain channelizer's (the kernel body is shared and promises that to every epilogue).
 *
 * A call of n samples with J = out_count(n) outputs per channel gives, per channel k,
 *
 *     e_k[m] = (double)re * (double)re + (double)im * (double)im        the two products are exact in double, the add rounds once
 *     sum[k] = sum over the call's J outputs of e_k[m]                   accumulated in double
 *
 * in this FIXED order (no floating-point atomics; nothing depends on timing, so the same stream behind reset gives the same
 * bits): a launch has W = min(tiles, grid) workgroups, tiles = ceil(J / tile_times); workgroup b takes the tiles b, b + W, ... in
 * that order and adds their outputs one by one, in time order, onto a partial sum that starts at +0; sum[k] is then
 * (((0 + partial_0) + partial_1) + ... + partial_{W-1}). Every e is >= 0, so any order is within (J - 1) 2^-53 of any other.
 * J = 0 (n < D can do that) gives sum[k] = 0 and leaves the levels and flags untouched; the count and the tail roll on as the
 * channelizer's do.
 *
 * State beyond the channelizer's count and tail. Per channel: level[k] (double), open[k] (0 or 1), the thresholds open_thr[k] and
 * close_thr[k] (doubles); and one counter `calls`, the calls with J > 0 since create or reset. A call with J > 0 does, per
 * channel and in this order (double arithmetic, evaluated as written, nothing fused):
 *
 *     mean     = sum[k] / J
 *     level[k] = mean                                        if calls == 0
 *              = level[k] + alpha * (mean - level[k])        otherwise
 *     open[k]  = !(level[k] < close_thr[k])                  if open[k] is set
 *              = level[k] >= open_thr[k]                     otherwise
 *
 * and then calls += 1. A NaN level — it follows from a NaN or an infinite input sample on a complex<float> row, which the
 * transform spreads to every channel — therefore changes no flag (both comparisons are false), and it stays until reset.
 *
 * Thresholds are absolute numbers in the units of |y|^2 that the host sets; at create every open_thr is +inf and every close_thr
 * 0, so no flag ever opens. The node estimates no noise floor.
 *
 * The kernels. chanpower_cs16_kernel / chanpower_cf32_kernel run the channelizer's phases 1 and 2 (channelizer_body.hpp) with a
 * third epilogue: no row is stored; lane `tid` owns the channels tid, tid + 256, ... and walks the tile's images in LDS
 * (consecutive lanes read consecutive words) adding e onto the workgroup's row of a [grid][M] double buffer — a read-modify-write
 * by the one lane that owns the element. The grid is bounded: `grid` is fixed at create, twice the device's compute units (the
 * environment knob SDRHIP_CHANPOWER_GRID=<n>, read at create, caps it: tests force the tile loop at small shapes with it), and
 * a workgroup loops over its tiles. chanpower_finish_kernel runs behind it on the same stream, one lane per channel: it adds the
 * rows of the workgroups that ran, writes sum[k] where asked and makes the level and flag update above.
 */
#ifndef SDRHIP_CHANPOWER_H
#define SDRHIP_CHANPOWER_H

#include "sdrhip_channelizer.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sdrhip_chanpower sdrhip_chanpower;

/* dtype, M, D, taps, n_taps, max_in: as sdrhip_channelizer_create takes them, with its rules, checked in its order and BEFORE
 * the context (host rules): NULL out / taps SDRHIP_E_INVALID; dtype SDRHIP_E_INVALID; M outside [2, 4096] SDRHIP_E_SIZE; M with a
 * prime factor above 13 SDRHIP_E_INVALID; D outside [1, M] SDRHIP_E_INVALID; n_taps outside [1, 64 M] SDRHIP_E_SIZE; max_in
 * outside [1, 2^30) SDRHIP_E_SIZE; a tap that is not finite as a float SDRHIP_E_INVALID; then alpha, the smoothing factor of the
 * level, outside (0, 1] — NaN included — SDRHIP_E_INVALID; then ctx = NULL: SDRHIP_E_NODEVICE on a machine without a usable
 * device, SDRHIP_E_INVALID elsewhere. */
int sdrhip_chanpower_create(sdrhip_ctx *ctx, int dtype, int M, int D, const double *taps, int n_taps, size_t max_in, double alpha,
                            sdrhip_chanpower **out);

/* the outputs per channel of a call of n samples made NOW: floor((N + n) / D) - floor(N / D), N the samples consumed so far */
int sdrhip_chanpower_out_count(sdrhip_chanpower *h, size_t n, size_t *n_out);

/* One row of n input elements in; sum: M doubles, the call's sums (zeros where J = 0); *n_out (may be NULL): J. Any n up to max_in
 * (above: SDRHIP_E_SIZE); n = 0 does nothing at all (sum is not written). _process_dev: sum_dev may be NULL where only the state is
 * wanted; two launches on the context's stream, nothing is synchronised; sum_dev must not overlap the input (SDRHIP_E_INVALID).
 * The kernel reads in[0 ... n) and the stored tail, nothing before or behind them. */
int sdrhip_chanpower_process_dev(sdrhip_chanpower *h, const void *in_dev, size_t n, double *sum_dev, size_t *n_out);
int sdrhip_chanpower_process(sdrhip_chanpower *h, const void *in_host, size_t n, double *sum_host, size_t *n_out);

/* M values each: 0 <= close_thr[k] <= open_thr[k], no NaN, +inf allowed for open_thr (else SDRHIP_E_INVALID, nothing changes).
 * Ordered on the context's stream behind the calls already enqueued. The flags are not looked at again until the next call with
 * J > 0. */
int sdrhip_chanpower_set_thresholds(sdrhip_chanpower *h, const double *open_thr, const double *close_thr);
/* a new smoothing factor in (0, 1] (else SDRHIP_E_INVALID, nothing changes), used from the next call on */
int sdrhip_chanpower_set_alpha(sdrhip_chanpower *h, double alpha);
/* a new prototype of the same length (n_taps doubles, rounded as at create; a tap that is not finite: SDRHIP_E_INVALID, nothing
 * changes); the count, the tail, the levels and the flags are kept. Ordered as set_thresholds is. */
int sdrhip_chanpower_set_taps(sdrhip_chanpower *h, const double *taps);
/* as freshly created (t = 0, a tail of zeros, every level 0, every flag 0, calls = 0), except that the current taps, alpha and
 * thresholds are kept */
int sdrhip_chanpower_reset(sdrhip_chanpower *h);
/* behind the calls enqueued so far: level[k] and open[k] of every channel. len >= M entries each (SDRHIP_E_SIZE); either pointer
 * may be NULL. */
int sdrhip_chanpower_get_levels(sdrhip_chanpower *h, double *level, unsigned char *open, int len);
/* behind the calls enqueued so far: the channels with open[k] == 1, ascending. *count is always their full number; at most cap
 * indices are written (idx may be NULL with cap = 0). With count >= 1 this is what sdrhip_channelizer_set_channels and
 * sdrhip_chanaudio_set_channels accept. */
int sdrhip_chanpower_get_occupied(sdrhip_chanpower *h, int *idx, int cap, int *count);
/* behind the calls enqueued so far: *consumed and tail as sdrhip_channelizer_get_state gives them (tail_len >= n_taps - 1 complex
 * elements where tail is given, SDRHIP_E_SIZE), and *calls, the calls with J > 0 since create or reset; any pointer may be NULL. */
int sdrhip_chanpower_get_state(sdrhip_chanpower *h, uint64_t *consumed, float *tail, size_t tail_len, uint64_t *calls);
/* the geometry of a launch, any pointer may be NULL: a workgroup takes tile_times consecutive output times at a time, every branch
 * sums branch_taps = ceil(n_taps / M) products, the workgroup's LDS images take lds_bytes, a launch has `grid` workgroups at most
 * (twice the compute units, the knob's cap, and never more than the tiles of a call of max_in samples), and their partial sums
 * take partial_bytes of device memory */
int sdrhip_chanpower_plan_info(sdrhip_chanpower *h, int *tile_times, int *branch_taps, int *lds_bytes, int *grid, int *partial_bytes);
/* "chanpower_cs16_kernel,chanpower_finish_kernel" or "chanpower_cf32_kernel,chanpower_finish_kernel": what a call launches */
int sdrhip_chanpower_kernel_names(sdrhip_chanpower *h, char *buf, size_t len);
int sdrhip_chanpower_destroy(sdrhip_chanpower *h);

#ifdef __cplusplus
}
#endif
#endif
