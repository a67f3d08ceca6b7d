/* sdrhip_chanaudio.h — the audio channelizer of libsdrhip.so: the polyphase channelizer of sdrhip_channelizer.h with a demodulator
 * per channel behind it, in the same launch: ONE antenna row to int16 AUDIO rows, one per selected channel, FM, AM or USB each.
 * The rows are what the symbol path takes (sdrhip_fmdeemph_bank_i16 -> the symbol detector bank -> the bit stream bank -> the
 * AX.25, POCSAG and Baudot banks), so a packet, pager or RTTY receiver on a uniform channel grid runs on the device at the
 * channelizer's cost instead of the tuner bank's. An addition to sdrhip.h and sdrhip_channelizer.h, which it includes; the error
 * codes, the dtype constants (SDRHIP_CHAN_CS16 / _CF32) and the conventions are theirs.
 *
 * The node has a definition of its own. For channel k, with mode[k] and gain[k], and output index m of the stream:
 *   1  y = y_k[m], the channelizer's output (sdrhip_channelizer.h), computed with the same operations in the same order as
 *      channelizer_*_kernel computes it: the same float32 bits.
 *   2  q = (conv(gain[k] * y.re), conv(gain[k] * y.im)), a complex<int16>: conv is ONE float32 multiply, then round to nearest
 *      even, NaN -> 0, clamp to [-32768, 32767] (so +-inf give the clamps). In numpy:
 *          np.clip(np.nan_to_num(np.rint(np.float32(g) * y32), nan=0), -32768, 32767).astype(np.int16)
 *   3  the reference's int16 demodulator on q, with the library's device functions (fm_phi, am_i16, usb_i16):
 *      AM  out = (int16) sqrt(re^2 + im^2)  (AMDemod<int16_t>),  USB  out = (re + im) / 2  (USBDemod<int16_t>): pointwise.
 *      FM  the library's per-call convention — that of sdrhip_demod_create(FM, cs16, inplace_fm0 = 1) and of the tuner bank.
 *          With j the output's index WITHIN THE CALL and phi[j] = fast_atan2(q.re, q.im) / 2 (FMDemod<int16_t>):
 *              out[0] = q[0].re;   for j >= 1: out[j] = (int16)(last - phi[j]), then last = phi[j].
 *          A call's sample 0 never touches `last`: a call of one output leaves it as it was, a call of n_out >= 2 outputs leaves
 *          phi[n_out - 1]. `last` is per channel, carried over calls, 0 at create and at reset.
 * AM and USB rows therefore do not depend on how the stream is cut into calls; FM rows do, at each call's first output only.
 *
 * Modes, gains and `last` are held PER CHANNEL k, all M of them, not per row: a selection (set_channels) only says which rows
 * are written. Every call moves `last` on for every FM channel, selected or not, so a channel that is deselected and selected
 * again — and any selected row — carries exactly what the same channel of the all-channels run carries, bit for bit. The
 * calls that name a `row` (set_mode, set_gain) and the arrays of get_modes, get_gains and get_state follow the CURRENT
 * selection: row i is channel idx[i] of the last set_channels (all M in order by default).
 *
 * Output layout: channel-major int16 rows, out_stride in int16 elements. Counts per call are the channelizer's:
 * floor((N + n) / D) - floor(N / D) per row; n = 0 and n < D are legal.
 *
 * The kernel (chanaudio_cs16_kernel / chanaudio_cf32_kernel): phases 1 and 2 are the channelizer's own (one shared body, so the
 * spectra agree bit for bit); the epilogue reads the tile's spectra from LDS, converts, demodulates and stores T contiguous
 * int16 per row. FM needs the angle of the output time before a tile's first one, which another workgroup computes: a tile that
 * does not begin the call, in a launch with at least one selected FM row, computes one more image for that time (the halo:
 * T + 1 images, LDS is sized for them). Tile 0 reads the old `last`; the workgroup holding output n_out - 1 writes every FM
 * channel's new one into the handle's OTHER buffer (as the tail is double-buffered: the blocks of a launch read the old one).
 */
#ifndef SDRHIP_CHANAUDIO_H
#define SDRHIP_CHANAUDIO_H

#include "sdrhip_channelizer.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sdrhip_chanaudio sdrhip_chanaudio;

/* dtype, M, D, taps, n_taps, max_in: as sdrhip_channelizer_create. modes: M entries, channel k's demodulator, each SDRHIP_EPI_FM,
 * _AM or _USB (NULL: every channel FM). gains: M floats, channel k's gain (NULL: every gain 1).
 * Errors, checked in this order and BEFORE the context (host rules): NULL out / taps SDRHIP_E_INVALID; then the rules of
 * sdrhip_channelizer_create in its order (dtype, M, M's factors, D, n_taps, max_in, taps); a mode that is SDRHIP_EPI_NONE
 * SDRHIP_E_UNSUPPORTED (complex<int16> rows are not made), any other value that is none of the three SDRHIP_E_INVALID — the
 * first offending channel answers; a gain that is not finite SDRHIP_E_INVALID; then ctx = NULL: SDRHIP_E_NODEVICE on a machine
 * without a usable device, SDRHIP_E_INVALID elsewhere. */
int sdrhip_chanaudio_create(sdrhip_ctx *ctx, int dtype, int M, int D, const double *taps, int n_taps, size_t max_in, const int *modes,
                            const float *gains, sdrhip_chanaudio **out);

/* the outputs per row of a call of n samples made NOW (sdrhip_channelizer_out_count) */
int sdrhip_chanaudio_out_count(sdrhip_chanaudio *h, size_t n, size_t *n_out);

/* One row of n input elements in; out: one int16 row per selected channel, out_stride in int16 elements (0 = the call's output
 * count; below it: SDRHIP_E_SIZE); *n_out (may be NULL): the outputs written per row. Any n up to max_in (above: SDRHIP_E_SIZE);
 * n = 0 does nothing. _process_dev: one launch on the context's stream, nothing is synchronised; the output extent must not overlap
 * the input's (SDRHIP_E_INVALID). A call that completes no block of D samples still launches: the tail moves on. */
int sdrhip_chanaudio_process_dev(sdrhip_chanaudio *h, const void *in_dev, size_t n, void *out_dev, size_t out_stride, size_t *n_out);
int sdrhip_chanaudio_process(sdrhip_chanaudio *h, const void *in_host, size_t n, void *out_host, size_t out_stride, size_t *n_out);

/* Every setter is ordered on the context's stream behind the calls already enqueued, and changes nothing where it fails.
 * set_channels: as sdrhip_channelizer_set_channels (idx = NULL: all M in order). Modes, gains and `last` belong to the channels
 * and stay with them (see the head of the file). */
int sdrhip_chanaudio_set_channels(sdrhip_chanaudio *h, const int *idx, int n_sel);
/* row's channel gets the demodulator `mode` and starts from last = 0 — also where the mode is the one it had (as
 * sdrhip_tunermodes_i16_set_mode). row outside [0, rows) SDRHIP_E_INVALID; SDRHIP_EPI_NONE SDRHIP_E_UNSUPPORTED; another
 * unknown mode SDRHIP_E_INVALID. */
int sdrhip_chanaudio_set_mode(sdrhip_chanaudio *h, int row, int mode);
int sdrhip_chanaudio_get_modes(sdrhip_chanaudio *h, int *modes, int n);     /* n >= rows (else SDRHIP_E_INVALID) */
/* row's channel gets the gain; `last` is kept. A gain that is not finite: SDRHIP_E_INVALID. */
int sdrhip_chanaudio_set_gain(sdrhip_chanaudio *h, int row, float gain);
int sdrhip_chanaudio_get_gains(sdrhip_chanaudio *h, float *gains, int n);   /* n >= rows */
int sdrhip_chanaudio_set_taps(sdrhip_chanaudio *h, const double *taps);     /* as sdrhip_channelizer_set_taps; `last` is kept */
/* as freshly created (t = 0, a tail of zeros, every last = 0), with the current taps, selection, modes and gains */
int sdrhip_chanaudio_reset(sdrhip_chanaudio *h);
/* behind the calls enqueued so far: *consumed and tail as sdrhip_channelizer_get_state gives them, and last[i], row i's `last`
 * (n_last >= rows where last is given, else SDRHIP_E_SIZE). Any pointer may be NULL. */
int sdrhip_chanaudio_get_state(sdrhip_chanaudio *h, uint64_t *consumed, float *tail, size_t tail_len, int *last, size_t n_last);
/* the geometry of a launch made now, any pointer may be NULL: tile_times, branch_taps and rows as sdrhip_channelizer_plan_info;
 * lds_bytes for tile_times + 1 images; fm_rows: the selected rows that are FM; halo_tiles: of a call of max_in samples from
 * the current count, the tiles that compute a halo image (0 where fm_rows is 0) */
int sdrhip_chanaudio_plan_info(sdrhip_chanaudio *h, int *tile_times, int *branch_taps, int *lds_bytes, int *rows, int *fm_rows,
                               int *halo_tiles);
/* "chanaudio_cs16_kernel" or "chanaudio_cf32_kernel": the one kernel every call of the handle runs (the FM halo is computed in
 * it; there is no differencing pass) */
int sdrhip_chanaudio_kernel_names(sdrhip_chanaudio *h, char *buf, size_t len);
int sdrhip_chanaudio_destroy(sdrhip_chanaudio *h);

#ifdef __cplusplus
}
#endif
#endif
