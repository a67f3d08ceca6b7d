/* sdr/gpu/pocsag.hh — gpu::POCSAGBank: N reference POCSAG nodes (src/pocsag.cc) behind the bit rows of a receiver.
 *
 * The reference runs pocsag_repair — a search over every 1- and 2-bit error pattern — on the window behind every bit a channel
 * receives while it waits for a sync word. This bank does the sync search and the word repair of all channels in one launch
 * (sdrhip_pocsag_*, include/sdrhip_pocsag.h) and keeps the reference's message rules on the host (pocsag_message.hh). Per
 * call: one sdrhip_pocsag_process_dev, one D2H copy of the event counts and event rows, then per channel the assembly; at
 * every END event of a channel handleMessages(channel) is called, with the channel's finished messages in queue(channel) —
 * the subclassing contract of the reference's POCSAG::handleMessages, per channel.
 */
#ifndef SDR_GPU_POCSAG_HH
#define SDR_GPU_POCSAG_HH

#include "receiver.hh"
#include "pocsag_message.hh"
#include "../../sdrhip_pocsag.h"

namespace sdr {
namespace gpu {

class POCSAGBank {
public:
  typedef pocsag::Message Message;

  /** channels nodes, all enabled; maxBits: the most bits a row brings per call (a receiver's bit-row capacity).
   * Throws ConfigError where there is no device or an argument is refused. */
  POCSAGBank(size_t channels, size_t maxBits, int device = 0)
    : _ctx(Device::get(device)), _C(channels), _maxBits(maxBits), _cap(sdrhip_pocsag_out_capacity(maxBits)),
      _hdr((channels * sizeof(uint32_t) + 15) & ~size_t(15)), _asm(channels) {
    std::vector<int> on(channels ? channels : 1, 1);
    detail::configCheck(sdrhip_pocsag_create(_ctx, on.data(), int(channels), maxBits, _h.out()), "POCSAGBank");
    _dev.alloc(_ctx, _hdr + _C * _cap * 2 * sizeof(uint32_t), "POCSAGBank");
    _host.resize((_hdr + _C * _cap * 2 * sizeof(uint32_t)) / sizeof(uint32_t));
  }
  virtual ~POCSAGBank() {
    sdrhip_ctx_synchronize(_ctx);
    _h.reset();
  }

  size_t channels() const { return _C; }
  size_t maxBits() const { return _maxBits; }

  /** Host rows: `channels` rows of `stride` bytes, row c holding counts[c] bits (bit 0 of each byte). */
  bool process(const uint8_t *bits, size_t stride, const uint32_t *counts) {
    uint32_t *h = _host.data();
    if (!detail::processOk(sdrhip_pocsag_process(_h, bits, stride, counts, h + _hdr / 4, _cap, h), "gpu::POCSAGBank")) return false;
    _assemble();
    return true;
  }
  /** Device rows and counts, as sdrhip_bits_process_dev and sdrhip_rxbank_process_dev leave them, on this bank's device. */
  bool processDev(const uint8_t *bitsDev, size_t stride, const uint32_t *countsDev) {
    uint32_t *d = _dev.as<uint32_t>();
    if (!detail::processOk(sdrhip_pocsag_process_dev(_h, bitsDev, stride, countsDev, d + _hdr / 4, _cap, d, 0), "gpu::POCSAGBank") ||
        !detail::processOk(sdrhip_memcpy_d2h_async(_ctx, _host.data(), _dev.get(), _host.size() * sizeof(uint32_t)), "gpu::POCSAGBank") ||
        !detail::processOk(sdrhip_ctx_synchronize(_ctx), "gpu::POCSAGBank"))
      return false;
    _assemble();
    return true;
  }
  /** The bit rows the receiver's last buffer left on the device (same device, same channel count), with no host copy. */
  bool process(const ReceiverBank<int16_t> &rx) {
    if (!rx.deviceBitRows()) return false;
    return processDev(rx.deviceBitRows(), rx.deviceBitStride(), rx.deviceBitCounts());
  }

  /** Called once per END of `channel`: queue(channel) holds the messages finished since that channel's last END. What is
   * left in the queue afterwards stays for the next call. */
  virtual void handleMessages(size_t channel) { (void)channel; }
  std::vector<Message> &queue(size_t channel) { return _asm[channel].queue(); }

  void setEnabled(size_t c, bool on) { detail::configCheck(sdrhip_pocsag_set_enabled(_h, int(c), on ? 1 : 0), "POCSAGBank"); }
  /** Every channel a freshly configured node, open messages and queues dropped; the enabled flags stay. */
  void reset() {
    detail::configCheck(sdrhip_pocsag_reset(_h), "POCSAGBank");
    for (size_t c = 0; c < _C; c++) _asm[c] = pocsag::Assembler();
  }
  void resetChannel(size_t c) {
    detail::configCheck(sdrhip_pocsag_reset_channel(_h, int(c)), "POCSAGBank");
    _asm[c] = pocsag::Assembler();
  }

protected:
  void _assemble() {
    const uint32_t *counts = _host.data(), *ev = _host.data() + _hdr / 4;
    for (size_t c = 0; c < _C; c++)
      for (size_t k = 0; k < counts[c] && k < _cap; k++)
        if (_asm[c].feed(ev[(c * _cap + k) * 2], ev[(c * _cap + k) * 2 + 1])) handleMessages(c);
  }

  sdrhip_ctx *_ctx;
  size_t _C, _maxBits, _cap, _hdr;   // _hdr: bytes of the counts in front of the event rows, device and host alike
  detail::Handle<sdrhip_pocsag, sdrhip_pocsag_destroy> _h;
  detail::DeviceMem _dev;
  std::vector<uint32_t> _host;
  std::vector<pocsag::Assembler> _asm;
};

}  // namespace gpu
}  // namespace sdr
#endif
