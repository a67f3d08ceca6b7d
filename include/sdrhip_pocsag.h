/* sdrhip_pocsag.h — the POCSAG decoder bank of libsdrhip.so: the bit rows of sdrhip_bits_process_dev / sdrhip_rxbank_process_dev
 * in, pager codewords out, on the device. An addition to sdrhip.h, which it includes; the error codes and conventions are
 * that header's.
 *
 * A handle holds `channels` independent POCSAG nodes of the reference (src/pocsag.cc:41-95), each with exactly that node's
 * state — the 64-bit shift register, WAIT / RECEIVE / CHECK_CONTINUE, the bit count, the slot — and an `enabled` flag.
 * What the reference does per bit on the host, this does per call on the device: the sync test of every bit position and the
 * BCH(31,21)+parity repair of every codeword (src/bch31_21.cc:123-212, here one look-up by the 11-bit syndrome). The message
 * assembly (_process_word, _finish_message, handleMessages) stays on the host and reads the EVENTS a call leaves:
 *
 *   an event is two uint32: word, info.   info [1:0]  kind: SDRHIP_POCSAG_SYNC, _WORD, _END
 *                                              [4:2]  slot 0 ... 7 (WORD only)
 *                                              [5]    repaired: the accepted word differs from the received one
 *                                              [31:8] index, within this call's row, of the bit that completed the event
 *   SYNC  WAIT -> RECEIVE (the reference resets its message here); word = 0x7CD215D8.
 *   WORD  one codeword for which pocsag_repair returned 0; word = the repaired word, slot = _slot at that moment. The first
 *         word of a slot precedes the second, both carry the same bit index. A sync or idle word seen in RECEIVE is a WORD like
 *         any other; an unrepairable word leaves no event.
 *   END   the failed continuation check (the reference runs _finish_message and handleMessages here); word = 0.
 *   A continuation check that succeeds leaves no event. The events of a row are in bit order.
 */
#ifndef SDRHIP_POCSAG_H
#define SDRHIP_POCSAG_H

#include "sdrhip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SDRHIP_POCSAG_SYNC 0
#define SDRHIP_POCSAG_WORD 1
#define SDRHIP_POCSAG_END 2
/* the node's _state, as sdrhip_pocsag_channel_state reports it */
#define SDRHIP_POCSAG_WAIT 0
#define SDRHIP_POCSAG_RECEIVE 1
#define SDRHIP_POCSAG_CHECK_CONTINUE 2

typedef struct sdrhip_pocsag sdrhip_pocsag;

/* enabled[c] != 0: row c decodes; 0: the row yields no event and its state is neither read nor written, so a row enabled again
 * goes on from the state it had. max_bits: the largest counts[c] of a call.
 * Errors, checked in this order and BEFORE the context (host rules): NULL enabled or out SDRHIP_E_INVALID; channels outside
 * 1 ... 8192 SDRHIP_E_INVALID; max_bits 0 or above 65536 SDRHIP_E_SIZE; then ctx = NULL: SDRHIP_E_NODEVICE on a machine
 * without a usable device, SDRHIP_E_INVALID elsewhere. */
int sdrhip_pocsag_create(sdrhip_ctx *ctx, const int *enabled, int channels, size_t max_bits, sdrhip_pocsag **out);

/* Events a row of n_bits bits can leave at most: n/32 + n/256 + 4 (integer division). At most two WORD events per 64 bits,
 * plus the word pair a carried-in bit count completes at the first bit; a SYNC and its END are at least 544 bits apart. */
size_t sdrhip_pocsag_out_capacity(size_t n_bits);

/* bits: channels rows of bits_stride bytes (0 = max_bits), counts: channels entries, as sdrhip_bits_process_dev and
 * sdrhip_rxbank_process_dev deliver them: row c holds counts[c] bits, bit 0 of a byte is the bit, and no byte at or behind
 * counts[c] is read. A counts[c] above max_bits is clamped to max_bits and *status is set to 1 (0 otherwise).
 * events: channels rows of ev_stride events (2 * ev_stride uint32); ev_stride >= sdrhip_pocsag_out_capacity(max_bits), 0 means
 * exactly that. ev_counts: channels entries; nothing is written behind ev_counts[c] events of row c.
 * status (may be NULL: the handle's own word, which only sdrhip_pocsag_process reads): one uint32 on the device.
 * One launch on the context's stream; nothing is synchronised. */
int sdrhip_pocsag_process_dev(sdrhip_pocsag *h, const uint8_t *bits_dev, size_t bits_stride, const uint32_t *counts_dev,
                              uint32_t *events_dev, size_t ev_stride, uint32_t *ev_counts_dev, uint32_t *status_dev);
/* the same with host pointers; the event bytes behind ev_counts[c] arrive as zeros. Where a count was clamped the call runs,
 * delivers its events and returns SDRHIP_E_SIZE. */
int sdrhip_pocsag_process(sdrhip_pocsag *h, const uint8_t *bits_host, size_t bits_stride, const uint32_t *counts_host,
                          uint32_t *events_host, size_t ev_stride, uint32_t *ev_counts_host);

/* Control calls: each is ordered on the context's stream behind the calls already enqueued.
 * _reset makes every row a freshly configured node (WAIT, every register 0) and keeps the flags; _reset_channel does that to
 * one row — the partner of sdrhip_bitsbank_set_channel — and touches no other. */
int sdrhip_pocsag_set_enabled(sdrhip_pocsag *h, int channel, int enabled);
int sdrhip_pocsag_get_enabled(sdrhip_pocsag *h, int *enabled, int n);   /* n >= channels */
int sdrhip_pocsag_reset(sdrhip_pocsag *h);
int sdrhip_pocsag_reset_channel(sdrhip_pocsag *h, int channel);
/* the reference node's protected state of row c after the calls enqueued so far; any out pointer may be NULL */
int sdrhip_pocsag_channel_state(sdrhip_pocsag *h, int channel, int *state, int *bitcount, int *slot, uint64_t *shift64);
int sdrhip_pocsag_kernel_names(sdrhip_pocsag *h, char *buf, size_t len);   /* "pocsag_decode_kernel" */
int sdrhip_pocsag_destroy(sdrhip_pocsag *h);

#ifdef __cplusplus
}
#endif
#endif
