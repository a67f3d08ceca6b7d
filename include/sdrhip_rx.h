/* sdrhip_rx.h — the receiver bank of libsdrhip.so: ONE antenna buffer in, every channel's bits out, nothing leaving the
 * device in between; and the per-channel FMDeemph<int16_t> it needs in the middle. An addition to sdrhip.h, which it
 * includes; the handles, error codes and conventions are that header's.
 *
 * The chain is the one every receiver of the reference runs (examples/sdr_ax25.cc, sdr_pocsag.cc, sdr_rtty.cc, sdr_rec.cc):
 *   antenna -> IQBaseBand -> FMDemod | AMDemod | USBDemod -> FMDeemph -> FSKDetector | ASKDetector -> BitStream
 *   tuner bank (sdrhip_tuner*_i16_create)                    deemph      detector (bank)             bits (bank)
 */
#ifndef SDRHIP_RX_H
#define SDRHIP_RX_H

#include "sdrhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- FMDeemph<int16_t> per channel ----------------------------------------------------------- */
/* `channels` FMDeemph<int16_t> nodes of one alpha (reference src/demod.hh:276-351), each enabled or not: enabled[c] != 0
 * is the node as configured, 0 the node after enable(false) — a pass-through (:328): the output row holds the input row's n
 * samples and the row's average is neither read nor written, so a row enabled again goes on from the average it had.
 * An enabled row is bit for bit what a handle of sdrhip_deemph_i16_create gives for that row alone.
 * The handle is a sdrhip_deemph: sdrhip_deemph_i16_process, _process_dev, _reset (every average zeroed, the flags kept),
 * _destroy and _kernel_names take it and keep their meaning. Kernels (kernel_names): "deemphbank_i16_copy_kernel" (alpha = 1),
 * "deemphbank_i16_seq_kernel", "deemphbank_i16_spec_kernel" — the BANK instances of the one-parameter handle's kernel
 * bodies, chosen by the same rule (in a profile: deemph_i16_*_kernel<true>, beside the one-parameter handle's <false>); a
 * mixed bank speculates wherever an all-enabled one does.
 * Errors, checked in this order and BEFORE the context (host rules): NULL enabled or out SDRHIP_E_INVALID; alpha outside
 * 1 ... 32767 SDRHIP_E_INVALID; channels outside 1 ... 8192 SDRHIP_E_INVALID; max_in SDRHIP_E_SIZE; then ctx = NULL:
 * SDRHIP_E_NODEVICE on a machine without a usable device, SDRHIP_E_INVALID elsewhere. */
int sdrhip_deemphbank_i16_create(sdrhip_ctx *ctx, int alpha, const int *enabled, int channels, size_t max_in, sdrhip_deemph **out);
/* enable(bool) of ONE row, between any two calls: ordered on the context's stream behind the calls already enqueued; no other
 * row is touched. On a handle of sdrhip_deemph_i16_create both calls return SDRHIP_E_UNSUPPORTED. */
int sdrhip_deemphbank_i16_set_enabled(sdrhip_deemph *h, int channel, int enabled);
int sdrhip_deemphbank_i16_get_enabled(sdrhip_deemph *h, int *enabled, int n);   /* n >= channels */

/* ---- receiver bank ---------------------------------------------------------------------------- */
/* Composes handles the caller made with the existing create calls: a tuner bank of any of the four forms whose rows are
 * demodulated int16 (SDRHIP_EPI_NONE rows are cs16: SDRHIP_E_UNSUPPORTED), optionally a de-emphasis handle (NULL: none),
 * a detector and a bit stream, each a bank or a one-parameter handle, all of the tuner's channel count and on `ctx`.
 * The receiver bank BORROWS them: they must outlive it and the caller destroys them afterwards. The caller keeps the
 * pointers, and every control call of a component — sdrhip_tuner_i16_set_shift / _set_taps, sdrhip_tunermodes_i16_set_mode,
 * sdrhip_detectorbank_set_channel, sdrhip_bitsbank_set_channel, sdrhip_deemphbank_i16_set_enabled, every reset — stays the
 * way to change a running receiver between two calls; the receiver bank has no setter of its own.
 * It owns the device rows between the stages. One call enqueues tuner -> de-emphasis -> detector -> bit stream on the
 * context's stream through the components' *_process_dev entry points, each stage out of place.
 * THE CALLER'S RULE: the bit stream's sample rate has to be the tuner's OUTPUT rate (input rate / decimation). The tuner
 * does not know its rate, so this cannot be checked here.
 * Create checks, in this order: a NULL tuner, detector, bits or out SDRHIP_E_INVALID; ctx = NULL SDRHIP_E_NODEVICE on a
 * machine without a usable device, SDRHIP_E_INVALID elsewhere; a component of another context SDRHIP_E_INVALID; a cs16
 * tuner SDRHIP_E_UNSUPPORTED; unequal channel counts SDRHIP_E_INVALID; a later stage whose max_in is below
 * ceil(tuner max_in / decimation) SDRHIP_E_SIZE. */
typedef struct sdrhip_rxbank sdrhip_rxbank;
int sdrhip_rxbank_create(sdrhip_ctx *ctx, sdrhip_tuner_i16 *tuner, sdrhip_deemph *deemph /* may be NULL */,
                         sdrhip_detector *detector, sdrhip_bits *bits, sdrhip_rxbank **out);
/* What the next call of n_in samples needs: n_audio = samples per audio row (the tuner's out_count), bits_cap = the bit
 * rows' smallest stride (sdrhip_bits_out_capacity of n_audio). Does not advance the state; either pointer may be NULL. */
int sdrhip_rxbank_sizes(sdrhip_rxbank *h, size_t n_in, size_t *n_audio, size_t *bits_cap);
/* in: ONE row of n_in antenna samples, as the tuner takes them. bits: channels rows of bits_stride bytes (0 = bits_cap of
 * this call), counts: channels entries — exactly what sdrhip_bits_process_dev delivers: row c holds counts[c] bits and
 * nothing is written behind them. audio (may be NULL): channels rows of audio_stride int16 (0 = n_audio of this call), the
 * rows the detector read — after the de-emphasis stage — *n_audio samples each (n_audio may be NULL).
 * n_in = 0, and a call whose tuner stage emits no sample, run no later stage: every count is 0 and *n_audio is 0 (an FM
 * channel's empty buffer produces nothing, as in the reference). */
int sdrhip_rxbank_process_dev(sdrhip_rxbank *h, const void *in_dev, size_t n_in, uint8_t *bits_dev, size_t bits_stride,
                              uint32_t *counts_dev, int16_t *audio_dev /* may be NULL */, size_t audio_stride, size_t *n_audio);
/* the same with host pointers; the bytes of a bit row behind counts[c] arrive as zeros */
int sdrhip_rxbank_process(sdrhip_rxbank *h, const void *in_host, size_t n_in, uint8_t *bits_host, size_t bits_stride,
                          uint32_t *counts_host, int16_t *audio_host /* may be NULL */, size_t audio_stride, size_t *n_audio);
int sdrhip_rxbank_destroy(sdrhip_rxbank *h);   /* the components stay */

#ifdef __cplusplus
}
#endif
#endif
