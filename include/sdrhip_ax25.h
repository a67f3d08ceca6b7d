/* sdrhip_ax25.h — the AX.25 deframer bank of libsdrhip.so: the bit rows of sdrhip_bits_process_dev / sdrhip_rxbank_process_dev in
 * (an APRS channel: FSKDetector(1200, 1200, 2200), BitStream(1200, TRANSITION)), checked frames out, on the device. An addition
 * to sdrhip.h, which it includes; the error codes and conventions are that header's.
 *
 * A handle holds `channels` independent AX25 nodes of the reference (src/ax25.hh, src/ax25.cc:79-161), each with exactly that
 * node's state — the 32-bit shift register _bitstream, _bitbuffer, _state, _rxbuffer[512] and the fill len = _ptr - _rxbuffer —
 * and an `enabled` flag. Per input byte b the node does
 *     _bitstream = (_bitstream << 1) | (b & 1);
 * and acts on the first rule that matches:
 *   flag     (_bitstream & 0xff) == 0x7e. With _state == 1 and len > 2 the CRC-CCITT of rxbuffer[0:len] is taken (init 0xffff,
 *            reflected, good residue 0xf0b8) and, if it is good, a frame of len - 2 bytes is delivered. Then _state = 1,
 *            len = 0, _bitbuffer = 0x80.
 *   abort    (_bitstream & 0x7f) == 0x7f: _state = 0.
 *   idle     _state == 0: nothing.
 *   stuffed  (_bitstream & 0x3f) == 0x3e: the bit is dropped.
 *   data     _bitbuffer |= bit << 8. With bit 0 of _bitbuffer set a byte is complete: with len >= 512 _state = 0 (the frame is
 *            lost, _bitbuffer stays as it is), otherwise the byte (_bitbuffer >> 1) & 0xff is stored and _bitbuffer = 0x80.
 *            Without it _bitbuffer >>= 1.
 * Two consequences, kept: the first bits of a closing flag are pushed as data bits before the flag is recognised at its eighth
 * bit (seven of them, or six when the flag's zero follows five ones and so counts as stuffed) — whole bytes only enter len and
 * the CRC; and after an overflow _bitbuffer keeps its stale value, 1 | byte << 1 of the byte that found no room, until the
 * next flag.
 *
 * What the reference does per bit on the host, this does for 64 bit positions at a time: the class of every
 * position from its own 8-bit window, the segments the flags cut a chunk into, the data bits of a segment compacted into a
 * word from which whole bytes shift out, a running CRC. The frames, the events, the counts and the state are bit-exact for any
 * split into calls.
 *
 * Three deviations.
 *   Out-of-bounds write. With len == 512 the reference's `*_ptr = 0` at a flag writes behind _rxbuffer. Nothing is written
 *   there here; the byte is not part of the CRC, so no output differs.
 *   Short frames. AX25::Message(buffer, length) subtracts 7 per address from a size_t without looking at length: a CRC-valid
 *   frame shorter than its address field makes the reference read behind the frame, or underflow. The deframer delivers such a
 *   frame raw, as any other; the host-side parsers (sdr/gpu/ax25_message.hh, libsdr_amd.ax25.Message) check the bounds, mark it
 *   malformed and do not parse it into addresses.
 *   Output capacity. Not the reference's buffer (it has none: it hands every frame to a virtual call) but two formulas:
 *     frames  a delivered frame has len >= 3, which takes 24 data positions behind the position that completed its opening
 *             flag, and one more completes the closing flag: two delivering flags lie 25 positions apart at least (the row
 *             flag, then 17 bits and a flag over and over meets that: the 17 bits and the flag's first seven are three bytes).
 *             A frame carried in can complete at position 0. So frames <= n_bits / 25 + 1 = sdrhip_ax25_frames_capacity.
 *     bytes   every buffered byte took eight data positions of this call or was carried in, at most 512 are carried in, and
 *             a frame delivers two bytes fewer than were buffered. The most n_bits >= 1 positions deliver is 510 — a carried
 *             frame closed at position 0 — plus max(0, (n_bits - 2) / 8 - 2) — one frame over everything between that flag
 *             and one completed by the last position. A row has room for sdrhip_ax25_bytes_capacity(n_bits) = n_bits / 8 +
 *             512: an upper bound of that for every n_bits, 0 included, 2 to 5 bytes above it.
 *   Nothing is written behind either, and no frame is dropped.
 */
#ifndef SDRHIP_AX25_H
#define SDRHIP_AX25_H

#include "sdrhip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SDRHIP_AX25_RXBUFFER 512   /* the node's _rxbuffer, and the caller's buffer of the two state calls */

typedef struct sdrhip_ax25 sdrhip_ax25;

/* `channels` nodes. enabled[c] != 0: row c deframes; 0: the row yields 0 frames and its state is neither read nor written, so a
 * row enabled again goes on from the state it had. enabled = NULL: every row. max_bits: the largest counts[c] of a call.
 * Errors, checked in this order and BEFORE the context (host rules): NULL out SDRHIP_E_INVALID; channels outside 1 ... 8192
 * SDRHIP_E_INVALID; max_bits 0 or above 65536 SDRHIP_E_SIZE; then ctx = NULL: SDRHIP_E_NODEVICE on a machine without a usable
 * device, SDRHIP_E_INVALID elsewhere. */
int sdrhip_ax25_create(sdrhip_ctx *ctx, const int *enabled, int channels, size_t max_bits, sdrhip_ax25 **out);

/* Frames a row of n_bits bits can deliver at most: n_bits / 25 + 1 (integer division). */
size_t sdrhip_ax25_frames_capacity(size_t n_bits);
/* Room for the frame bytes a row of n_bits bits can deliver: n_bits / 8 + 512. */
size_t sdrhip_ax25_bytes_capacity(size_t n_bits);

/* bits: channels rows of bits_stride bytes (0 = max_bits), counts: channels entries, as sdrhip_bits_process_dev and
 * sdrhip_rxbank_process_dev deliver them: row c holds counts[c] bits, bit 0 of a byte is the bit, and no byte at or behind
 * counts[c] is read. A counts[c] above max_bits is clamped to max_bits and *status is set to 1 (0 otherwise).
 * bytes: channels rows of bytes_stride bytes; bytes_stride >= sdrhip_ax25_bytes_capacity(max_bits), 0 means exactly that. The
 *   frames a row delivered, back to back, the FCS stripped.
 * events: channels rows of ev_stride events of two uint32; ev_stride >= sdrhip_ax25_frames_capacity(max_bits), 0 means exactly
 *   that. One event per delivered frame, in bit order: word 0 the byte offset of the frame in the row's bytes, word 1
 *   length | bit_index << 16 — the length 1 ... 510, the bit index that of the bit, within this call's row, that completed
 *   the closing flag.
 * frame_counts: channels entries. Nothing is written behind frame_counts[c] events of row c, nor behind the bytes they name.
 * status (may be NULL: the handle's own word, which only sdrhip_ax25_process reads): one uint32 on the device.
 * One launch on the context's stream; nothing is synchronised. */
int sdrhip_ax25_process_dev(sdrhip_ax25 *h, const uint8_t *bits_dev, size_t bits_stride, const uint32_t *counts_dev, uint8_t *bytes_dev,
                            size_t bytes_stride, uint32_t *events_dev, size_t ev_stride, uint32_t *frame_counts_dev, uint32_t *status_dev);
/* the same with host pointers; the bytes and events behind a row's frames arrive as zeros. Where a count was clamped the call
 * runs, delivers its frames and returns SDRHIP_E_SIZE. */
int sdrhip_ax25_process(sdrhip_ax25 *h, const uint8_t *bits_host, size_t bits_stride, const uint32_t *counts_host, uint8_t *bytes_host,
                        size_t bytes_stride, uint32_t *events_host, size_t ev_stride, uint32_t *frame_counts_host);

/* Control calls: each is ordered on the context's stream behind the calls already enqueued.
 * _reset / _reset_channel make every row / one row a freshly configured node (config(): both registers and _state 0, the buffer
 * empty). The flags stay. */
int sdrhip_ax25_set_enabled(sdrhip_ax25 *h, int channel, int enabled);
int sdrhip_ax25_get_enabled(sdrhip_ax25 *h, int *enabled, int n);   /* n >= channels */
int sdrhip_ax25_reset(sdrhip_ax25 *h);
int sdrhip_ax25_reset_channel(sdrhip_ax25 *h, int channel);
/* the reference node's protected state of row c after the calls enqueued so far; any out pointer may be NULL. rxbuffer: room for
 * SDRHIP_AX25_RXBUFFER bytes, of which the first *len are written. */
int sdrhip_ax25_channel_state(sdrhip_ax25 *h, int channel, uint32_t *bitstream, uint32_t *bitbuffer, int *state, int *len, uint8_t *rxbuffer);
/* puts a node into that state, one the node can reach: state 0 or 1, len 0 ... 512 (rxbuffer may be NULL with len 0), and with
 * state 1 a _bitbuffer of 1 ... 0xff (a marker bit below the bits of the byte under way); anything else SDRHIP_E_INVALID. The
 * running CRC of rxbuffer[0:len], which the kernel carries beside the node's members, is recomputed here. */
int sdrhip_ax25_set_channel_state(sdrhip_ax25 *h, int channel, uint32_t bitstream, uint32_t bitbuffer, int state, int len, const uint8_t *rxbuffer);
int sdrhip_ax25_kernel_names(sdrhip_ax25 *h, char *buf, size_t len);   /* "ax25_deframe_kernel" */
int sdrhip_ax25_destroy(sdrhip_ax25 *h);

#ifdef __cplusplus
}
#endif
#endif
