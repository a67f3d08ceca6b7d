/* sdr/gpu/receiver.hh — gpu::ReceiverBank<int16_t>: one antenna to every channel's bits, as one node.
 *
 * The reference's receivers all run antenna -> IQBaseBand -> FMDemod / AMDemod / USBDemod -> FMDeemph -> FSKDetector /
 * ASKDetector -> BitStream (examples/sdr_ax25.cc, sdr_pocsag.cc, sdr_rtty.cc, sdr_rec.cc), one chain per channel. This node is
 * N such chains on one antenna: a Sink<cs16> whose every stage serves all channels in one launch and whose rows never leave
 * the device between the stages (sdrhip_rxbank_*, include/sdrhip_rx.h). Per input buffer: one H2D copy, one
 * sdrhip_rxbank_process_dev, one D2H copy of the counts and the bit rows into a pinned staging buffer — and one of the audio
 * rows, only while some audio(c) has a sink.
 */
#ifndef SDR_GPU_RECEIVER_HH
#define SDR_GPU_RECEIVER_HH

#include "nodes.hh"
#include "../../sdrhip_rx.h"

namespace sdr {
namespace gpu {

template <class Scalar> class ReceiverBank;

/** A tuner bank with a demodulator per channel (it IS a gpu::TunerBank<int16_t>(PerChannel): addChannel's tunes, setMode,
 * setCenterFrequency, setFilterFrequency and setFilterWidth are that bank's, bookkeeping included) whose channels each carry
 * a service: what to detect, at which baud rate, how to read the bits, de-emphasis or not.
 *   bits(c)   a Source configured as gpu::BitStream configures its own: uint8, rate = baud, buffer = that channel's
 *             capacity; it sends head(count), and only when a buffer produced at least one bit (src/fsk.cc:201)
 *   audio(c)  a Source of int16 at the decimated rate: the rows the detector read (after the de-emphasis stage). An FM
 *             channel sends nothing for an empty buffer, as FMDemod does
 * The outputs are views of the node's staging buffers: while a consumer still holds one of the last round, this round is
 * dropped (the rule of TunerBank::process). addChannel() after config() rebuilds every stage: all channels restart as
 * freshly configured nodes. setService / enableDeemph / setMode and the tune setters change ONE channel of the running
 * receiver between two buffers; the other channels stream on. */
template <>
class ReceiverBank<int16_t> : public detail::TunerBank16<detail::ComplexBank> {
  typedef detail::TunerBank16<detail::ComplexBank> Base;

public:
  struct Service {
    enum Kind { FSK, ASK };
    Kind kind;
    float baud, mark, space;   // mark / space: FSK only
    bool invert;               // ASK only
    BitStream::Mode mode;
    bool deemph;
    /** FSKDetector(baud, Fmark, Fspace) -> BitStream(baud, mode) */
    static Service fsk(float baud, float Fmark, float Fspace, BitStream::Mode mode = BitStream::TRANSITION, bool deemph = false) {
      Service s = {FSK, baud, Fmark, Fspace, false, mode, deemph};
      return s;
    }
    /** ASKDetector<int16_t>(invert) -> BitStream(baud, mode) */
    static Service ask(float baud, bool invert = false, BitStream::Mode mode = BitStream::NORMAL, bool deemph = false) {
      Service s = {ASK, baud, 0.f, 0.f, invert, mode, deemph};
      return s;
    }
  };

  /** maxSymbolsPerBit: the longest correlator / bit window a later setService may ask for (audio rate / baud, at most 2048). */
  ReceiverBank(size_t order, size_t sub_sample, int device = 0, size_t maxSymbolsPerBit = 2048)
    : Base(order, sub_sample, Base::PerChannel, device), _maxL(maxSymbolsPerBit), _M(0), _cap(0), _hdr(0) {}
  virtual ~ReceiverBank() {
    _release();
    for (size_t c = 0; c < _bitOuts.size(); c++) delete _bitOuts[c];
  }

  /** A new channel; returns its index. Before or after config(). A bad mode or service throws ConfigError and adds nothing. */
  size_t addChannel(double Fc, double Ff, double width, int mode, const Service &service) {
    _checkService(service);
    _checkMode(mode);
    _services.push_back(service);
    _bitOuts.push_back(new Out());
    return Base::addChannel(Fc, Ff, width, mode);   // (rebuilds a configured bank: _rebuild below)
  }
  const Service &service(size_t c) const { return _services[c]; }
  Source *bits(size_t c) { return _bitOuts[c]; }
  Source *audio(size_t c) { return this->source(c); }

  /** Read-only: the bit rows of the last processed buffer as they lie on the device — rows of deviceBitStride() bytes, row c
   * holding deviceBitCounts()[c] bits (a device array too) — for a node that goes on from them there (gpu::POCSAGBank).
   * Null before config(); valid until the next buffer, setService or addChannel. */
  const uint8_t *deviceBitRows() const { return _rx ? _dbits.as<uint8_t>() + _hdr : 0; }
  size_t deviceBitStride() const { return _cap; }
  const uint32_t *deviceBitCounts() const { return _rx ? _dbits.as<uint32_t>() : 0; }

  /** Channel c's detector and bit stream become freshly configured nodes (sdrhip_detectorbank_set_channel,
   * sdrhip_bitsbank_set_channel), its de-emphasis is switched as the service says; bits(c) is configured anew. */
  void setService(size_t c, const Service &service) {
    _checkService(service);
    if (_rx) {
      if (double(_audioRate()) / service.baud >= double(_maxL + 1) || double(_audioRate()) / service.baud < 1.0) {
        ConfigError err;
        err << "ReceiverBank: " << service.baud << " baud at " << _audioRate() << " Hz is outside 1 ... " << _maxL << " symbols per bit";
        throw err;
      }
      _setDetector(c, service);
      detail::configCheck(sdrhip_bitsbank_set_channel(_bits, int(c), service.baud, _bitMode(service)), "ReceiverBank");
      detail::configCheck(sdrhip_deemphbank_i16_set_enabled(_deemph, int(c), service.deemph ? 1 : 0), "ReceiverBank");
      _services[c] = service;
      _stageBitRows();
      _configureBits(c);
    } else _services[c] = service;
  }
  /** FMDeemph::enable of channel c: off is a pass-through and the average rests; on again continues from it. */
  void enableDeemph(size_t c, bool on) {
    if (_rx) detail::configCheck(sdrhip_deemphbank_i16_set_enabled(_deemph, int(c), on ? 1 : 0), "ReceiverBank");
    _services[c].deemph = on;
  }

  virtual void process(const Buffer<cs16> &b, bool) {
    if (!_rx || b.size() > _bs || b.size() == 0) return;
    if (!_stageOut.isUnused() || !_stageBits.isUnused()) {
      LogMessage msg(LOG_WARNING);
      msg << "gpu::ReceiverBank: output of the last round still in use downstream; buffer dropped";
      Logger::get().log(msg);
      return;
    }
    const size_t C = _tunes.size(), astride = 2 * _outStride;   // int16 elements of a row of _dout / _stageOut
    bool wantAudio = false;
    for (size_t c = 0; c < C && !wantAudio; c++) wantAudio = _outs[c]->connected();
    size_t n = 0;
    uint8_t *dbits = _dbits.as<uint8_t>();
    if (!detail::processOk(sdrhip_memcpy_h2d_async(_ctx, _din.get(), b.data(), b.size() * sizeof(cs16)), "gpu::ReceiverBank") ||
        !detail::processOk(sdrhip_rxbank_process_dev(_rx, _din.get(), b.size(), dbits + _hdr, _cap, _dbits.as<uint32_t>(),
                                                     wantAudio ? _dout.as<int16_t>() : 0, astride, &n), "gpu::ReceiverBank") ||
        !detail::processOk(sdrhip_memcpy_d2h_async(_ctx, _stageBits.data(), dbits, _hdr + C * _cap), "gpu::ReceiverBank") ||
        (wantAudio && n &&
         !detail::processOk(sdrhip_memcpy_d2h_async(_ctx, _stageOut.data(), _dout.get(), C * _outStride * sizeof(cs16)), "gpu::ReceiverBank")) ||
        !detail::processOk(sdrhip_ctx_synchronize(_ctx), "gpu::ReceiverBank"))
      return;
    const uint32_t *counts = reinterpret_cast<const uint32_t *>(_stageBits.data());
    for (size_t c = 0; c < C; c++) {
      if (wantAudio) detail::sendDemodulated(*_outs[c], _modes[c], _stageOut, c * _outStride, n, false);
      if (counts[c]) _bitOuts[c]->send(_stageBits.sub(_hdr + c * _cap, counts[c]), false);   // src/fsk.cc:201
    }
  }

protected:
  typedef ChannelBank<int16_t>::Out Out;

  static int _bitMode(const Service &s) { return s.mode == BitStream::TRANSITION ? SDRHIP_BITS_TRANSITION : SDRHIP_BITS_NORMAL; }
  double _audioRate() const { return detail::ComplexBank::outRate(_Fs, _D); }

  static void _checkService(const Service &s) {
    const bool kind = s.kind == Service::FSK || s.kind == Service::ASK;
    const bool mode = s.mode == BitStream::NORMAL || s.mode == BitStream::TRANSITION;
    if (kind && mode && s.baud > 0) return;
    ConfigError err;
    err << "ReceiverBank: bad service (kind " << int(s.kind) << ", baud " << s.baud << ", bit mode " << int(s.mode) << ")";
    throw err;
  }

  /** the LUTs of one FSK service at the audio rate, as gpu::FSKDetector designs them */
  void _fskLuts(const Service &s, std::vector<float> &mark, std::vector<float> &space, int &L) const {
    L = design::fskCorrLen(_audioRate(), s.baud);
    mark.resize(2 * size_t(std::max(L, 0)));
    space.resize(mark.size());
    design::fskLut(_audioRate(), s.mark, L, mark.data());
    design::fskLut(_audioRate(), s.space, L, space.data());
  }
  void _setDetector(size_t c, const Service &s) {
    if (s.kind == Service::ASK) {
      detail::configCheck(sdrhip_detectorbank_set_channel(_det, int(c), SDRHIP_DET_ASK, 0, 0, 0, s.invert ? 1 : 0), "ReceiverBank");
      return;
    }
    std::vector<float> mark, space;
    int L = 0;
    _fskLuts(s, mark, space, L);
    detail::configCheck(sdrhip_detectorbank_set_channel(_det, int(c), SDRHIP_DET_FSK, mark.data(), space.data(), L, 0), "ReceiverBank");
  }

  void _configureBits(size_t c) {
    size_t cap = 0;
    detail::configCheck(sdrhip_bitsbank_channel_info(_bits, int(c), _M, 0, 0, 0, &cap), "ReceiverBank");
    _bitOuts[c]->configure(Config(Config::typeId<uint8_t>(), _services[c].baud, cap, 1));   // as gpu::BitStream: src/fsk.cc:154
  }

  /** The device block [counts: C x uint32, padded to 16 bytes][C bit rows of the bank's largest capacity] and its pinned host
   * mirror; allocated anew when a faster service raised the capacity. */
  void _stageBitRows() {
    size_t cap = 0;
    detail::configCheck(sdrhip_bits_out_capacity(_bits, _M, &cap), "ReceiverBank");
    if (cap <= _cap) return;
    if (!_stageBits.isUnused()) {
      ConfigError err;
      err << "ReceiverBank: the bit rows have to grow while a consumer still holds the last round's";
      throw err;
    }
    const size_t C = _tunes.size();
    if (_ctx) sdrhip_ctx_synchronize(_ctx);
    _pinBits.reset();
    _stageBits.unref();
    _cap = cap;
    _hdr = (C * sizeof(uint32_t) + 15) & ~size_t(15);
    _dbits.alloc(_ctx, _hdr + C * _cap, "ReceiverBank");
    _stageBits = Buffer<uint8_t>(_hdr + C * _cap);
    _pinBits.reset(_stageBits.data(), _hdr + C * _cap, "ReceiverBank");
  }

  /** The receiver bank goes before its components, those before the tuner's buffers. */
  virtual void _release() {
    if (_ctx) sdrhip_ctx_synchronize(_ctx);
    _rx.reset();
    _bits.reset();
    _det.reset();
    _deemph.reset();
    _dbits.reset();
    _pinBits.reset();
    _stageBits.unref();
    _cap = 0;
    Base::_release();
  }

  virtual void _rebuild() {
    Base::_rebuild();   // (releases everything first; then the tuner bank, its input row and — as the audio rows — its output rows)
    const size_t C = _tunes.size();
    if (!_plan) return;
    _M = (_bs + _D - 1) / _D;
    const double rate = _audioRate();
    std::vector<int> kinds(C), lens(C), inv(C), modes(C), deemph(C);
    std::vector<float> marks, spaces, bauds(C), m, s;
    for (size_t c = 0; c < C; c++) {
      const Service &sv = _services[c];
      kinds[c] = sv.kind == Service::FSK ? SDRHIP_DET_FSK : SDRHIP_DET_ASK;
      inv[c] = sv.invert ? 1 : 0;
      bauds[c] = sv.baud; modes[c] = _bitMode(sv); deemph[c] = sv.deemph ? 1 : 0;
      if (sv.kind != Service::FSK) continue;
      _fskLuts(sv, m, s, lens[c]);
      marks.insert(marks.end(), m.begin(), m.end());
      spaces.insert(spaces.end(), s.begin(), s.end());
    }
    detail::configCheck(sdrhip_deemphbank_i16_create(_ctx, design::fmDeemphAlpha(rate), deemph.data(), int(C), _M, _deemph.out()), "ReceiverBank");
    detail::configCheck(sdrhip_detectorbank_create(_ctx, kinds.data(), lens.data(), inv.data(), marks.empty() ? 0 : marks.data(),
                                                   spaces.empty() ? 0 : spaces.data(), int(_maxL), int(C), _M, _det.out()), "ReceiverBank");
    detail::configCheck(sdrhip_bitsbank_create(_ctx, rate, bauds.data(), modes.data(), int(C), _M, int(_maxL), _bits.out()), "ReceiverBank");
    detail::configCheck(sdrhip_rxbank_create(_ctx, _plan, _deemph, _det, _bits, _rx.out()), "ReceiverBank");
    _stageBitRows();
    for (size_t c = 0; c < C; c++) _configureBits(c);
  }

  size_t _maxL, _M, _cap, _hdr;
  std::vector<Service> _services;
  std::vector<Out *> _bitOuts;
  detail::Handle<sdrhip_deemph, sdrhip_deemph_i16_destroy> _deemph;
  detail::Handle<sdrhip_detector, sdrhip_detector_destroy> _det;
  detail::Handle<sdrhip_bits, sdrhip_bits_destroy> _bits;
  detail::Handle<sdrhip_rxbank, sdrhip_rxbank_destroy> _rx;
  detail::DeviceMem _dbits;
  detail::Pinned _pinBits;   // the registration of _stageBits
  Buffer<uint8_t> _stageBits;
};

}  // namespace gpu
}  // namespace sdr
#endif
