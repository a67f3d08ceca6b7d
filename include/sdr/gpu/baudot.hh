/* sdr/gpu/baudot.hh — gpu::Baudot, the drop-in for the reference's Baudot node (src/baudot.hh, src/baudot.cc): the half-bit
 * stream of a BitStream(90.90) in, text out — the third stage of an RTTY receiver — and gpu::BaudotBank, N such nodes behind the
 * bit rows of a receiver bank in one launch (sdrhip_baudot_*, include/sdrhip_baudot.h).
 *
 * One deviation from the reference: its output buffer, bufferSize / (2 * bitsPerSymbol) + 1 characters, is about half of what
 * a buffer of continuous traffic completes, and it is indexed unchecked. gpu::Baudot declares and owns bufferSize / 14 + 1
 * characters, the most any stop-bit setting can complete; no text is dropped and nothing is written behind the buffer.
 */
#ifndef SDR_GPU_BAUDOT_HH
#define SDR_GPU_BAUDOT_HH

#include "receiver.hh"
#include "../../sdrhip_baudot.h"

namespace sdr {
namespace gpu {

/** Baudot(stopBits) with the reference's surface. The constructor sets LETTERS; config() zeroes the two registers and — as the
 * reference's does — keeps the table when it is called again (sdrhip_baudot_reset with keep_mode = 1; a larger buffer makes a
 * new device node that starts in the old one's table). process() sends only when at least one character was decoded. */
class Baudot : public Sink<uint8_t>, public Source {
public:
  typedef enum { LETTERS, FIGURES } Mode;
  typedef enum { STOP1, STOP15, STOP2 } StopBits;

  Baudot(StopBits stopBits = STOP15, int device = 0) : _stopBits(stopBits), _device(device), _maxBits(0), _cap(0), _configured(false) {}
  virtual ~Baudot() { _buffer.unref(); }

  virtual void config(const Config &src_cfg) {
    if (!src_cfg.hasType()) return;
    detail::checkType<uint8_t>(src_cfg, "Baudot");
    const size_t bs = std::max(size_t(1), src_cfg.bufferSize());
    if (_configured && bs <= _maxBits) {
      resetPlan();
    } else {
      const Mode m = _configured ? planMode() : LETTERS;
      createPlan(bs, m);
      _maxBits = bs;
      _configured = true;
    }
    _cap = bs / 14 + 1;
    _stage.assign(_maxBits / 14 + 1, 0);
    _buffer.unref();
    _buffer = Buffer<uint8_t>(_cap);
    LogMessage msg(LOG_DEBUG);
    msg << "Config Baudot node: " << std::endl
        << " input sample rate: " << src_cfg.sampleRate() << " half-bits/s" << std::endl
        << " start bits: " << 1 << std::endl
        << " stop bits: " << float(2 + int(_stopBits)) / 2;
    Logger::get().log(msg);
    this->setConfig(Config(Config::typeId<uint8_t>(), 0, _cap, 1));
  }

  virtual void process(const Buffer<uint8_t> &buffer, bool allow_overwrite) {
    (void)allow_overwrite;
    if (!_plan) return;
    const uint32_t n = uint32_t(buffer.size());
    uint32_t o = 0;
    if (!detail::processOk(sdrhip_baudot_process(_plan, reinterpret_cast<const uint8_t *>(buffer.data()), 0, &n, _stage.data(), _stage.size(), &o), "gpu::Baudot")) return;
    if (0 == o) return;
    if (!_buffer.isUnused()) return;   // still referenced downstream: the text of this buffer is dropped
    o = uint32_t(std::min(size_t(o), _cap));
    memcpy(_buffer.data(), _stage.data(), o);
    this->send(_buffer.head(o));
  }

  /** The table the node is in behind the buffers processed so far. */
  Mode mode() const { return _configured ? const_cast<Baudot *>(this)->planMode() : LETTERS; }

protected:
  /** A fresh device node for buffers of up to maxBits half-bits, starting in table `mode`. */
  virtual void createPlan(size_t maxBits, Mode mode) {
    detail::configCheck(sdrhip_baudot_create(Device::get(_device), int(_stopBits), 1, maxBits, _plan.out()), "Baudot");
    if (mode != LETTERS) detail::configCheck(sdrhip_baudot_set_channel_state(_plan, 0, 0, 0, SDRHIP_BAUDOT_FIGURES), "Baudot");
  }
  /** config() on the old node: the registers start over, the table stays. */
  virtual void resetPlan() { detail::configCheck(sdrhip_baudot_reset(_plan, 1), "Baudot"); }
  virtual Mode planMode() {
    int m = SDRHIP_BAUDOT_LETTERS;
    detail::configCheck(sdrhip_baudot_channel_state(_plan, 0, 0, 0, &m), "Baudot");
    return m == SDRHIP_BAUDOT_FIGURES ? FIGURES : LETTERS;
  }

  StopBits _stopBits;
  int _device;
  size_t _maxBits, _cap;
  bool _configured;
  detail::Handle<sdrhip_baudot, sdrhip_baudot_destroy> _plan;
  std::vector<uint8_t> _stage;
  Buffer<uint8_t> _buffer;
};

/** N Baudot nodes over bit rows, host or device. Not a graph node: process() takes `channels` host rows, processDev() the
 * device rows and counts a gpu::ReceiverBank call (or sdrhip_bits_process_dev) left on this bank's device, with no host copy
 * of the bits in between; text(c) is what row c decoded in the last call. */
class BaudotBank {
public:
  typedef Baudot::StopBits StopBits;

  /** channels nodes of one setting, all enabled; maxBits: the most half-bits a row brings per call (a receiver's bit-row
   * capacity). Throws ConfigError where there is no device or an argument is refused. */
  BaudotBank(size_t channels, size_t maxBits, StopBits stopBits = Baudot::STOP15, int device = 0)
    : _ctx(Device::get(device)), _C(channels), _maxBits(maxBits) {
    detail::configCheck(sdrhip_baudot_create(_ctx, int(stopBits), int(channels), maxBits, _h.out()), "BaudotBank");
    _alloc();
  }
  /** A setting per row. */
  BaudotBank(const std::vector<StopBits> &stopBits, size_t maxBits, int device = 0)
    : _ctx(Device::get(device)), _C(stopBits.size()), _maxBits(maxBits) {
    std::vector<int> s(_C ? _C : 1, 0);
    for (size_t c = 0; c < _C; c++) s[c] = int(stopBits[c]);
    detail::configCheck(sdrhip_baudotbank_create(_ctx, s.data(), 0, int(_C), maxBits, _h.out()), "BaudotBank");
    _alloc();
  }
  virtual ~BaudotBank() {
    sdrhip_ctx_synchronize(_ctx);
    _h.reset();
  }

  size_t channels() const { return _C; }
  size_t maxBits() const { return _maxBits; }

  /** Host rows: `channels` rows of `stride` bytes, row c holding counts[c] half-bits (bit 0 of each byte). */
  bool process(const uint8_t *bits, size_t stride, const uint32_t *counts) {
    uint8_t *h = _host.data();
    return detail::processOk(sdrhip_baudot_process(_h, bits, stride, counts, h + _hdr, _cap, reinterpret_cast<uint32_t *>(h)), "gpu::BaudotBank");
  }
  /** Device rows and counts, as sdrhip_bits_process_dev and sdrhip_rxbank_process_dev leave them, on this bank's device. */
  bool processDev(const uint8_t *bitsDev, size_t stride, const uint32_t *countsDev) {
    uint8_t *d = _dev.as<uint8_t>();
    return detail::processOk(sdrhip_baudot_process_dev(_h, bitsDev, stride, countsDev, d + _hdr, _cap, reinterpret_cast<uint32_t *>(d), 0),
                             "gpu::BaudotBank") &&
           detail::processOk(sdrhip_memcpy_d2h_async(_ctx, _host.data(), _dev.get(), _host.size()), "gpu::BaudotBank") &&
           detail::processOk(sdrhip_ctx_synchronize(_ctx), "gpu::BaudotBank");
  }
  /** The bit rows the receiver's last buffer left on the device (same device, same channel count), with no host copy. */
  bool process(const ReceiverBank<int16_t> &rx) {
    if (!rx.deviceBitRows()) return false;
    return processDev(rx.deviceBitRows(), rx.deviceBitStride(), rx.deviceBitCounts());
  }

  /** What row `channel` decoded in the last call (a 0 byte — the null code — is a character like any other). */
  std::string text(size_t channel) const {
    const uint32_t n = std::min(reinterpret_cast<const uint32_t *>(_host.data())[channel], uint32_t(_cap));
    return std::string(reinterpret_cast<const char *>(_host.data() + _hdr + channel * _cap), n);
  }

  /** A freshly constructed node of another setting behind row c. */
  void setChannel(size_t c, StopBits stopBits) { detail::configCheck(sdrhip_baudot_set_channel(_h, int(c), int(stopBits)), "BaudotBank"); }
  void setEnabled(size_t c, bool on) { detail::configCheck(sdrhip_baudot_set_enabled(_h, int(c), on ? 1 : 0), "BaudotBank"); }
  /** Every row a freshly constructed node; keepMode: the registers start over, the tables stay. The flags stay. */
  void reset(bool keepMode = false) { detail::configCheck(sdrhip_baudot_reset(_h, keepMode ? 1 : 0), "BaudotBank"); }
  void resetChannel(size_t c, bool keepMode = false) { detail::configCheck(sdrhip_baudot_reset_channel(_h, int(c), keepMode ? 1 : 0), "BaudotBank"); }

protected:
  void _alloc() {
    _cap = sdrhip_baudot_out_capacity(_maxBits);
    _hdr = (_C * sizeof(uint32_t) + 15) & ~size_t(15);
    _dev.alloc(_ctx, _hdr + _C * _cap, "BaudotBank");
    _host.assign(_hdr + _C * _cap, 0);
  }

  sdrhip_ctx *_ctx;
  size_t _C, _maxBits, _cap, _hdr;   // _hdr: bytes of the counts in front of the text rows, device and host alike
  detail::Handle<sdrhip_baudot, sdrhip_baudot_destroy> _h;
  detail::DeviceMem _dev;
  std::vector<uint8_t> _host;
};

}  // namespace gpu
}  // namespace sdr
#endif
