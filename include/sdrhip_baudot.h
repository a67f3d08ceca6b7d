/* sdrhip_baudot.h — the Baudot decoder bank of libsdrhip.so: the half-bit rows of sdrhip_bits_process_dev /
 * sdrhip_rxbank_process_dev in (an RTTY channel at 90.90 half-bits per second), text out, on the device. An addition to
 * sdrhip.h, which it includes; the error codes and conventions are that header's.
 *
 * A handle holds `channels` independent Baudot nodes of the reference (src/baudot.hh, src/baudot.cc:86-111), each with exactly
 * that node's state — the 16-bit shift register _bitstream, the bit count _bitcount (kept exact, as a 64-bit count) and the
 * table _mode — a stop-bit setting and an `enabled` flag. Per input byte b the node does
 *     _bitstream = (_bitstream << 1) | (b & 1);  _bitcount++;
 * and takes a symbol when bitsPerSymbol <= _bitcount and (_bitstream & mask) == pattern:
 *
 *     setting              stopHBits  bitsPerSymbol  pattern  mask
 *     SDRHIP_BAUDOT_STOP1      2          14         0x3000   0x3003
 *     SDRHIP_BAUDOT_STOP15     3          15         0x6000   0x6007
 *     SDRHIP_BAUDOT_STOP2      4          16         0xC000   0xC00F
 *
 * A taken symbol sets _bitcount = 0; its 5-bit code has bit j = bit (stopHBits + 2 j) of _bitstream, j = 0 ... 4.
 *   code 31  the table becomes LETTERS, nothing is emitted;    code 27  the table becomes FIGURES, nothing is emitted;
 *   code 4   the table becomes LETTERS, then a space is emitted (a space ends a figures run);
 *   every other code emits one byte from the current table — code 0 a 0 byte (as do the table places of 27 and 31):
 *     code      0  1  2  3  4  5  6  7  8  9 10 11 12 13 14 15 16 17 18 19 20 21 22 23 24 25 26 27 28 29 30 31
 *     LETTERS  \0  E \n  A SP  S  I  U \n  D  R  J  N  F  C  K  T  Z  L  W  H  Y  P  Q  O  B  G \0  M  X  V \0
 *     FIGURES  \0  3 \n  - SP \a  8  7 \n  ?  4  '  ,  !  :  (  5  "  )  2  #  6  0  1  9  ?  & \0  .  /  ; \0
 * What the reference does per bit on the host, this does for 64 bit positions at a time: the pattern test of every position,
 * the gate "bitsPerSymbol bits since the last symbol" as a greedy pick over the mask of matching positions, and the table of
 * every symbol from the shift codes in front of it. The text, the counts and the state are bit-exact for any split into calls.
 *
 * One deviation, the output capacity. The reference sizes its output buffer bufferSize / (2 * bitsPerSymbol) + 1, but symbols
 * can complete every bitsPerSymbol half-bits, about twice that; on continuous traffic it writes behind its buffer. A row here
 * has room for sdrhip_baudot_out_capacity(n_bits) = n_bits / 14 + 1 characters, the most any setting can complete in n_bits
 * half-bits; nothing is written behind it and no text is dropped.
 */
#ifndef SDRHIP_BAUDOT_H
#define SDRHIP_BAUDOT_H

#include "sdrhip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SDRHIP_BAUDOT_STOP1 0
#define SDRHIP_BAUDOT_STOP15 1
#define SDRHIP_BAUDOT_STOP2 2
/* the node's _mode, as sdrhip_baudot_channel_state reports it */
#define SDRHIP_BAUDOT_LETTERS 0
#define SDRHIP_BAUDOT_FIGURES 1

typedef struct sdrhip_baudot sdrhip_baudot;

/* `channels` nodes with the stop-bit setting `stop`, every row enabled. max_bits: the largest counts[c] of a call.
 * Errors, checked in this order and BEFORE the context (host rules): NULL out SDRHIP_E_INVALID; stop not one of the three
 * settings SDRHIP_E_INVALID; channels outside 1 ... 8192 SDRHIP_E_INVALID; max_bits 0 or above 65536 SDRHIP_E_SIZE; then
 * ctx = NULL: SDRHIP_E_NODEVICE on a machine without a usable device, SDRHIP_E_INVALID elsewhere. */
int sdrhip_baudot_create(sdrhip_ctx *ctx, int stop, int channels, size_t max_bits, sdrhip_baudot **out);
/* A setting per row, stops[c], and a flag per row: enabled[c] != 0: row c decodes; 0: the row yields a count of 0 and its
 * state is neither read nor written, so a row enabled again goes on from the state it had. enabled = NULL: every row.
 * Errors, in this order and before the context: NULL stops or out SDRHIP_E_INVALID; channels outside 1 ... 8192
 * SDRHIP_E_INVALID; max_bits 0 or above 65536 SDRHIP_E_SIZE; a stops[c] that is not one of the three settings
 * SDRHIP_E_INVALID; then the context as above. */
int sdrhip_baudotbank_create(sdrhip_ctx *ctx, const int *stops, const int *enabled, int channels, size_t max_bits, sdrhip_baudot **out);

/* Characters a row of n_bits half-bits can leave at most: n_bits / 14 + 1 (integer division). */
size_t sdrhip_baudot_out_capacity(size_t n_bits);

/* bits: channels rows of bits_stride bytes (0 = max_bits), counts: channels entries, as sdrhip_bits_process_dev and
 * sdrhip_rxbank_process_dev deliver them: row c holds counts[c] half-bits, bit 0 of a byte is the half-bit, and no byte at or
 * behind counts[c] is read. A counts[c] above max_bits is clamped to max_bits and *status is set to 1 (0 otherwise).
 * text: channels rows of text_stride bytes; text_stride >= sdrhip_baudot_out_capacity(max_bits), 0 means exactly that.
 * out_counts: channels entries; nothing is written behind out_counts[c] characters of row c.
 * status (may be NULL: the handle's own word, which only sdrhip_baudot_process reads): one uint32 on the device.
 * One launch on the context's stream; nothing is synchronised. */
int sdrhip_baudot_process_dev(sdrhip_baudot *h, const uint8_t *bits_dev, size_t bits_stride, const uint32_t *counts_dev,
                              uint8_t *text_dev, size_t text_stride, uint32_t *out_counts_dev, uint32_t *status_dev);
/* the same with host pointers; the bytes behind out_counts[c] arrive as zeros. Where a count was clamped the call runs,
 * delivers its text and returns SDRHIP_E_SIZE. */
int sdrhip_baudot_process(sdrhip_baudot *h, const uint8_t *bits_host, size_t bits_stride, const uint32_t *counts_host,
                          uint8_t *text_host, size_t text_stride, uint32_t *out_counts_host);

/* Control calls: each is ordered on the context's stream behind the calls already enqueued.
 * _set_channel replaces the node behind one row with a freshly constructed one of setting `stop` — LETTERS, both registers 0 —
 * and touches no other row and no flag: the partner of sdrhip_bitsbank_set_channel.
 * _reset / _reset_channel: keep_mode 0 makes every row / one row a freshly constructed node of its setting; keep_mode != 0 is
 * the reference's config() on the old node: both registers 0, the table kept. The flags stay. */
int sdrhip_baudot_set_channel(sdrhip_baudot *h, int channel, int stop);
int sdrhip_baudot_set_enabled(sdrhip_baudot *h, int channel, int enabled);
int sdrhip_baudot_get_channels(sdrhip_baudot *h, int *stops, int *enabled, int n);   /* n >= channels; either array may be NULL */
int sdrhip_baudot_reset(sdrhip_baudot *h, int keep_mode);
int sdrhip_baudot_reset_channel(sdrhip_baudot *h, int channel, int keep_mode);
/* the reference node's protected state of row c after the calls enqueued so far; any out pointer may be NULL */
int sdrhip_baudot_channel_state(sdrhip_baudot *h, int channel, uint16_t *bitstream, uint64_t *bitcount, int *mode);
/* puts a node into that state (mode: SDRHIP_BAUDOT_LETTERS or _FIGURES, anything else SDRHIP_E_INVALID) */
int sdrhip_baudot_set_channel_state(sdrhip_baudot *h, int channel, uint16_t bitstream, uint64_t bitcount, int mode);
int sdrhip_baudot_kernel_names(sdrhip_baudot *h, char *buf, size_t len);   /* "baudot_decode_kernel" */
int sdrhip_baudot_destroy(sdrhip_baudot *h);

#ifdef __cplusplus
}
#endif
#endif
