/* sdr/gpu/channelizer.hh — gpu::Channelizer<Scalar>: the polyphase channelizer (sdrhip_channelizer_*, include/sdrhip_channelizer.h
 * has the contract) as a graph node: a Sink of std::complex<Scalar> — ONE antenna stream — with one Source per selected channel
 * (source(i), the ChannelBank::Out pattern), each emitting Buffer<std::complex<float>> at sampleRate / D. Scalar is int16_t or
 * float. The node has no reference node behind it: the reference has no way to split one stream into a uniform grid of channels
 * short of a baseband node per channel.
 *
 * Per buffer: one H2D copy, one launch for all channels, one D2H copy of all rows into a pinned staging buffer, then one send
 * per row, in row order, as views of it; a buffer that completes no block of D samples sends nothing. processDev() runs the
 * same plan on device rows of the node's device and synchronises nothing: its rows drop into the processDev of the banks that
 * take complex float rows (gpu::InpolSubSamplerBank, the BPSK31 and AGC banks).
 */
#ifndef SDR_GPU_CHANNELIZER_HH
#define SDR_GPU_CHANNELIZER_HH

#include "nodes.hh"
#include "../../sdrhip_channelizer.h"

#include <cmath>
#include <vector>

namespace sdr {
namespace gpu {

namespace detail {
template <class Scalar> struct ChannelizerType;
template <> struct ChannelizerType<int16_t> { enum { dtype = SDRHIP_CHAN_CS16 }; };
template <> struct ChannelizerType<float> { enum { dtype = SDRHIP_CHAN_CF32 }; };
}  // namespace detail

template <class Scalar>
class Channelizer : public Sink< std::complex<Scalar> > {
public:
  typedef std::complex<Scalar> In;
  typedef ChannelBank<int16_t>::Out Out;

  /** M channels decimated by D with the prototype low-pass `taps`; channels: the channels to deliver, any order, no duplicates
   * (empty: all M in order). The rules of sdrhip_channelizer_create are checked here and throw ConfigError: 2 <= M <= 4096 with
   * prime factors up to 13, 1 <= D <= M, 1 <= taps.size() <= 64 M, every tap finite as a float, every channel in [0, M), once. */
  Channelizer(size_t M, size_t D, const std::vector<double> &taps, const std::vector<int> &channels = std::vector<int>(), int device = 0)
    : Sink<In>(), _M(M), _D(D), _taps(taps), _sel(channels), _device(device), _ctx(0), _bs(0), _outStride(0) {
    size_t rest = M;
    const size_t primes[] = {2, 3, 5, 7, 11, 13};
    for (size_t q = 0; q < 6; q++) while (rest > 1 && rest % primes[q] == 0) rest /= primes[q];
    bool finite = true;
    for (size_t i = 0; i < taps.size(); i++) finite = finite && std::isfinite(float(taps[i]));
    if (M < 2 || M > 4096 || rest != 1 || D < 1 || D > M || taps.empty() || taps.size() > 64 * M || !finite) {
      ConfigError err;
      err << "Can not configure Channelizer node: M = " << M << " (2 ... 4096, prime factors up to 13), D = " << D << " (1 ... M), "
          << taps.size() << " taps (1 ... 64 M, all finite as floats)";
      throw err;
    }
    if (_sel.empty()) for (size_t k = 0; k < M; k++) _sel.push_back(int(k));
    std::vector<bool> seen(M, false);
    for (size_t i = 0; i < _sel.size(); i++) {
      if (_sel[i] < 0 || size_t(_sel[i]) >= M || seen[size_t(_sel[i])]) {
        ConfigError err;
        err << "Can not configure Channelizer node: channel " << _sel[i] << " (row " << i << ") is outside [0, " << M << ") or selected twice";
        throw err;
      }
      seen[size_t(_sel[i])] = true;
    }
    for (size_t i = 0; i < _sel.size(); i++) _outs.push_back(new Out());
  }
  virtual ~Channelizer() {
    _release();
    for (size_t i = 0; i < _outs.size(); i++) delete _outs[i];
  }

  /** The rows delivered, and the channel row i holds. */
  size_t rows() const { return _sel.size(); }
  int channel(size_t i) const { return _sel[i]; }
  Source *source(size_t i) { return _outs[i]; }
  sdrhip_ctx *context() const { return _ctx; }
  /** The smallest row stride of processDev: the most outputs a buffer of the configured size gives. */
  size_t outStride() const { return _outStride; }

  virtual void config(const Config &cfg) {
    if (!cfg.hasType() || !cfg.hasSampleRate() || !cfg.hasBufferSize()) return;
    detail::checkType<In>(cfg, "Channelizer node");
    _release();
    _bs = cfg.bufferSize();
    if (_bs == 0) return;
    _ctx = Device::get(_device);
    detail::configCheck(sdrhip_channelizer_create(_ctx, detail::ChannelizerType<Scalar>::dtype, int(_M), int(_D), _taps.data(), int(_taps.size()),
                                                  _bs, _plan.out()), "Channelizer");
    detail::configCheck(sdrhip_channelizer_set_channels(_plan, _sel.data(), int(_sel.size())), "Channelizer");
    _outStride = (_bs + _D - 1) / _D;
    const size_t R = _sel.size();
    _din.alloc(_ctx, _bs * sizeof(In), "Channelizer");
    _dout.alloc(_ctx, R * _outStride * sizeof(cf32), "Channelizer");
    _stageOut = Buffer<cf32>(R * _outStride);
    _pinOut.reset(_stageOut.data(), R * _outStride * sizeof(cf32), "Channelizer");
    for (size_t i = 0; i < R; i++) _outs[i]->configure(Config(Config::typeId<cf32>(), cfg.sampleRate() / double(_D), _outStride, 1));
  }

  virtual void process(const Buffer<In> &b, bool) {
    if (!_plan || b.size() > _bs || b.size() == 0) return;
    // the per-row outputs are views of _stageOut: while a consumer still holds one of the last round, this round is dropped
    if (!_stageOut.isUnused()) {
      LogMessage msg(LOG_WARNING);
      msg << "gpu::Channelizer: output of the last round still in use downstream; buffer dropped";
      Logger::get().log(msg);
      return;
    }
    const size_t R = _sel.size();
    size_t n = 0;
    if (!detail::processOk(sdrhip_memcpy_h2d_async(_ctx, _din.get(), b.data(), b.size() * sizeof(In)), "gpu::Channelizer") ||
        !detail::processOk(sdrhip_channelizer_process_dev(_plan, _din.get(), b.size(), _dout.get(), _outStride, &n), "gpu::Channelizer") ||
        !detail::processOk(sdrhip_memcpy_d2h_async(_ctx, _stageOut.data(), _dout.get(), R * _outStride * sizeof(cf32)), "gpu::Channelizer") ||
        !detail::processOk(sdrhip_ctx_synchronize(_ctx), "gpu::Channelizer"))
      return;
    if (n == 0) return;
    for (size_t i = 0; i < R; i++) _outs[i]->emit(_stageOut.sub(i * _outStride, n), false);
  }

  /** One row of n device samples in, rows() device rows out (outStride in complex floats, at least the call's output count);
   * one launch on the context's stream, nothing is synchronised. After config() only. */
  bool processDev(const void *inDev, size_t n, void *outDev, size_t outStride, size_t *nOut) {
    return detail::processOk(sdrhip_channelizer_process_dev(_plan, inDev, n, outDev, outStride, nOut), "gpu::Channelizer");
  }
  /** A new prototype of the same length; the stream goes on. */
  void setTaps(const std::vector<double> &taps) {
    if (taps.size() != _taps.size()) {
      ConfigError err;
      err << "Channelizer: " << taps.size() << " taps where the node has " << _taps.size();
      throw err;
    }
    if (_plan) detail::configCheck(sdrhip_channelizer_set_taps(_plan, taps.data()), "Channelizer");
    _taps = taps;
  }
  void reset() { if (_plan) detail::configCheck(sdrhip_channelizer_reset(_plan), "Channelizer"); }
  /** The samples taken since config() or reset(). */
  uint64_t consumed() const {
    uint64_t c = 0;
    if (_plan) detail::configCheck(sdrhip_channelizer_get_state(_plan, &c, 0, 0), "Channelizer");
    return c;
  }

protected:
  /** In this order: the device is idle before anything it may still use goes. */
  void _release() {
    if (_ctx) sdrhip_ctx_synchronize(_ctx);
    _plan.reset();
    _din.reset();
    _dout.reset();
    _pinOut.reset();
    _stageOut.unref();
  }

  size_t _M, _D;
  std::vector<double> _taps;
  std::vector<int> _sel;
  int _device;
  sdrhip_ctx *_ctx;
  detail::Handle<sdrhip_channelizer, sdrhip_channelizer_destroy> _plan;
  detail::DeviceMem _din, _dout;
  detail::Pinned _pinOut;   // the registration of _stageOut
  size_t _bs, _outStride;
  std::vector<Out *> _outs;
  Buffer<cf32> _stageOut;
};

}  // namespace gpu
}  // namespace sdr
#endif
