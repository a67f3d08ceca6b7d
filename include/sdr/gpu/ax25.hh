/* sdr/gpu/ax25.hh — gpu::AX25, the drop-in for the reference's AX25 node (src/ax25.hh, src/ax25.cc): the bit stream of a
 * BitStream(1200, TRANSITION) in, a virtual handleAX25Message(const Message &) per CRC-checked frame — the last stage of a packet
 * radio / APRS receiver — gpu::AX25Dump, which prints them, and gpu::AX25Bank, N such nodes behind the bit rows of a receiver bank
 * in one launch (sdrhip_ax25_*, include/sdrhip_ax25.h).
 *
 * The deviations are the header's: nothing is written behind _rxbuffer; a frame shorter than its address field reaches
 * handleAX25Message as a malformed() Message with its raw bytes (ax25_message.hh), where the reference reads behind the frame;
 * and the frames of a buffer are staged in rows of the header's two capacities.
 */
#ifndef SDR_GPU_AX25_HH
#define SDR_GPU_AX25_HH

#include <ostream>

#include "receiver.hh"
#include "ax25_message.hh"
#include "../../sdrhip_ax25.h"

namespace sdr {
namespace gpu {

/** AX25() with the reference's surface: a Sink<uint8_t> that hands every frame of a buffer to handleAX25Message, in bit order.
 * config() is the reference's: silent while the type is unknown, a ConfigError on another type than uint8_t, and a node that
 * starts over (both registers and _state 0, the buffer empty) every time it is called. */
class AX25 : public Sink<uint8_t> {
public:
  typedef ax25::Address Address;
  typedef ax25::Message Message;

  explicit AX25(int device = 0) : _device(device), _maxBits(0), _fcap(0), _bcap(0) {}
  virtual ~AX25() {}

  virtual void config(const Config &src_cfg) {
    if (!src_cfg.hasType()) return;
    detail::checkType<uint8_t>(src_cfg, "AX25");
    const size_t bs = std::max(size_t(1), src_cfg.bufferSize());
    if (_maxBits && bs <= _maxBits) {
      resetPlan();
    } else {
      createPlan(bs);
      _maxBits = bs;
      _fcap = sdrhip_ax25_frames_capacity(bs);
      _bcap = sdrhip_ax25_bytes_capacity(bs);
      _bytes.assign(_bcap, 0);
      _events.assign(2 * _fcap, 0);
    }
    LogMessage msg(LOG_DEBUG);
    msg << "Config AX.25 node.";
    Logger::get().log(msg);
  }

  virtual void process(const Buffer<uint8_t> &buffer, bool allow_overwrite) {
    (void)allow_overwrite;
    if (!_plan) return;
    const uint32_t n = uint32_t(buffer.size());
    uint32_t frames = 0;
    if (!detail::processOk(sdrhip_ax25_process(_plan, reinterpret_cast<const uint8_t *>(buffer.data()), 0, &n, _bytes.data(), _bcap, _events.data(),
                                               _fcap, &frames), "gpu::AX25")) return;
    for (uint32_t i = 0; i < frames && i < _fcap; i++) {
      const size_t at = _events[2 * i], len = _events[2 * i + 1] & 0xffffu;
      if (at + len > _bcap) break;
      this->handleAX25Message(Message(_bytes.data() + at, len));
    }
  }

  virtual void handleAX25Message(const Message &message) { (void)message; }

protected:
  /** A fresh device node for buffers of up to maxBits bits. */
  virtual void createPlan(size_t maxBits) { detail::configCheck(sdrhip_ax25_create(Device::get(_device), 0, 1, maxBits, _plan.out()), "AX25"); }
  /** config() on the old node. */
  virtual void resetPlan() { detail::configCheck(sdrhip_ax25_reset(_plan), "AX25"); }

  int _device;
  size_t _maxBits, _fcap, _bcap;
  detail::Handle<sdrhip_ax25, sdrhip_ax25_destroy> _plan;
  std::vector<uint8_t> _bytes;
  std::vector<uint32_t> _events;
};

/** Prints received AX25 messages to the specified stream, as the reference's AX25Dump does. */
class AX25Dump : public AX25 {
public:
  explicit AX25Dump(std::ostream &stream, int device = 0) : AX25(device), _stream(stream) {}
  virtual void handleAX25Message(const Message &message) { _stream << "AX25: " << message << std::endl; }

protected:
  std::ostream &_stream;
};

/** N AX25 nodes over bit rows, host or device. Not a graph node: process() takes `channels` host rows, processDev() the device
 * rows and counts a gpu::ReceiverBank call (or sdrhip_bits_process_dev) left on this bank's device, with no host copy of the bits
 * in between; frameCount(c), message(c, i) and bitIndex(c, i) are what row c delivered in the last call. */
class AX25Bank {
public:
  typedef ax25::Address Address;
  typedef ax25::Message Message;

  /** channels nodes, all enabled; maxBits: the most bits a row brings per call (a receiver's bit-row capacity). Throws
   * ConfigError where there is no device or an argument is refused. */
  AX25Bank(size_t channels, size_t maxBits, int device = 0) : _ctx(Device::get(device)), _C(channels), _maxBits(maxBits) {
    detail::configCheck(sdrhip_ax25_create(_ctx, 0, int(channels), maxBits, _h.out()), "AX25Bank");
    _fcap = sdrhip_ax25_frames_capacity(_maxBits);
    _bcap = sdrhip_ax25_bytes_capacity(_maxBits);
    _ev = (_C * sizeof(uint32_t) + 15) & ~size_t(15);
    _by = _ev + _C * _fcap * 2 * sizeof(uint32_t);
    _dev.alloc(_ctx, _by + _C * _bcap, "AX25Bank");
    _host.assign(_by + _C * _bcap, 0);
  }
  virtual ~AX25Bank() {
    sdrhip_ctx_synchronize(_ctx);
    _h.reset();
  }

  size_t channels() const { return _C; }
  size_t maxBits() const { return _maxBits; }

  /** Host rows: `channels` rows of `stride` bytes, row c holding counts[c] bits (bit 0 of each byte). */
  bool process(const uint8_t *bits, size_t stride, const uint32_t *counts) {
    uint8_t *h = _host.data();
    return detail::processOk(sdrhip_ax25_process(_h, bits, stride, counts, h + _by, _bcap, reinterpret_cast<uint32_t *>(h + _ev), _fcap,
                                                 reinterpret_cast<uint32_t *>(h)), "gpu::AX25Bank");
  }
  /** Device rows and counts, as sdrhip_bits_process_dev and sdrhip_rxbank_process_dev leave them, on this bank's device. */
  bool processDev(const uint8_t *bitsDev, size_t stride, const uint32_t *countsDev) {
    uint8_t *d = _dev.as<uint8_t>();
    return detail::processOk(sdrhip_ax25_process_dev(_h, bitsDev, stride, countsDev, d + _by, _bcap, reinterpret_cast<uint32_t *>(d + _ev), _fcap,
                                                     reinterpret_cast<uint32_t *>(d), 0), "gpu::AX25Bank") &&
           detail::processOk(sdrhip_memcpy_d2h_async(_ctx, _host.data(), _dev.get(), _host.size()), "gpu::AX25Bank") &&
           detail::processOk(sdrhip_ctx_synchronize(_ctx), "gpu::AX25Bank");
  }
  /** The bit rows the receiver's last buffer left on the device (same device, same channel count), with no host copy. */
  bool process(const ReceiverBank<int16_t> &rx) {
    if (!rx.deviceBitRows()) return false;
    return processDev(rx.deviceBitRows(), rx.deviceBitStride(), rx.deviceBitCounts());
  }

  /** The frames row `channel` delivered in the last call. */
  size_t frameCount(size_t channel) const { return std::min(size_t(reinterpret_cast<const uint32_t *>(_host.data())[channel]), _fcap); }
  /** Frame i of them, parsed (malformed() where its address field does not fit). */
  Message message(size_t channel, size_t i) const {
    const uint32_t *e = _event(channel, i);
    const size_t at = e[0], len = e[1] & 0xffffu;
    if (at + len > _bcap) return Message();
    return Message(_host.data() + _by + channel * _bcap + at, len);
  }
  /** The index, within the last call's row, of the bit that completed frame i's closing flag. */
  size_t bitIndex(size_t channel, size_t i) const { return _event(channel, i)[1] >> 16; }

  void setEnabled(size_t c, bool on) { detail::configCheck(sdrhip_ax25_set_enabled(_h, int(c), on ? 1 : 0), "AX25Bank"); }
  /** Every row / one row a freshly configured node. The flags stay. */
  void reset() { detail::configCheck(sdrhip_ax25_reset(_h), "AX25Bank"); }
  void resetChannel(size_t c) { detail::configCheck(sdrhip_ax25_reset_channel(_h, int(c)), "AX25Bank"); }

protected:
  const uint32_t *_event(size_t channel, size_t i) const {
    return reinterpret_cast<const uint32_t *>(_host.data() + _ev) + (channel * _fcap + i) * 2;
  }

  sdrhip_ctx *_ctx;
  size_t _C, _maxBits, _fcap, _bcap, _ev, _by;   // _ev, _by: where the event rows and the byte rows start, device and host alike
  detail::Handle<sdrhip_ax25, sdrhip_ax25_destroy> _h;
  detail::DeviceMem _dev;
  std::vector<uint8_t> _host;
};

}  // namespace gpu
}  // namespace sdr
#endif
