/* sdr/gpu/chanaudio.hh — gpu::AudioChannelizer<Scalar>: the audio channelizer (sdrhip_chanaudio_*, include/sdrhip_chanaudio.h has
 * the contract) as a graph node, shaped as gpu::Channelizer<Scalar>: a Sink of std::complex<Scalar> — ONE antenna stream — with
 * one Source per selected channel (source(i)), each emitting Buffer<int16_t> AUDIO at sampleRate / D: the channelizer's output
 * times the row's gain, rounded to complex<int16>, through the row's demodulator (FM, AM or USB). Scalar is int16_t or float.
 *
 * Per buffer: one H2D copy, one launch for all channels, one D2H copy of all rows into a pinned staging buffer, then one send
 * per row, in row order, as views of it; a buffer that completes no block of D samples sends nothing. processDev() runs the
 * same plan on device rows of the node's device and synchronises nothing: its rows drop into the processDev of the symbol path
 * (the de-emphasis bank, the detector bank, the bit stream bank, the frame decoders).
 *
 * The node's body is gpu::AudioChannelizerNode<Grid>, as gpu::ChannelizerNode is gpu::Channelizer's: Grid says what the complex
 * node and the real-input one of chanreal.hh (gpu::RealAudioChannelizer<Scalar>) differ in.
 */
#ifndef SDR_GPU_CHANAUDIO_HH
#define SDR_GPU_CHANAUDIO_HH

#include "channelizer.hh"
#include "../../sdrhip_chanaudio.h"

#include <cmath>
#include <string>
#include <vector>

namespace sdr {
namespace gpu {

namespace detail {
/** The complex audio node's grid: detail::ComplexGrid with sdrhip_chanaudio_create (modes and gains: one per channel). */
template <class Scalar> struct ComplexAudioGrid : ComplexGrid<Scalar> {
  static const char *name() { return "AudioChannelizer"; }
  static int create(sdrhip_ctx *ctx, int M, int D, const double *taps, int nTaps, size_t maxIn, const int *modes, const float *gains,
                    sdrhip_chanaudio **out) {
    return sdrhip_chanaudio_create(ctx, ChannelizerType<Scalar>::dtype, M, D, taps, nTaps, maxIn, modes, gains, out);
  }
};
}  // namespace detail

template <class Grid>
class AudioChannelizerNode : public Sink<typename Grid::In> {
public:
  typedef typename Grid::In In;
  typedef ChannelBank<int16_t>::Out Out;

  /** M, D, taps, channels, modes and gains as gpu::AudioChannelizer and gpu::RealAudioChannelizer say; the grid's rules are
   * checked here and throw ConfigError. */
  AudioChannelizerNode(size_t M, size_t D, const std::vector<double> &taps, const std::vector<int> &channels, const std::vector<int> &modes,
                       const std::vector<float> &gains, int device)
    : Sink<In>(), _M(M), _K(Grid::admitsM(M) ? Grid::channels(M) : 0), _D(D), _taps(taps), _sel(channels), _modes(modes), _gains(gains),
      _device(device), _ctx(0), _bs(0), _outStride(0), _gpuName(std::string("gpu::") + Grid::name()) {
    size_t rest = Grid::admitsM(M) ? Grid::transform(M) : 0;
    const size_t primes[] = {2, 3, 5, 7, 11, 13};
    for (size_t q = 0; q < 6; q++) while (rest > 1 && rest % primes[q] == 0) rest /= primes[q];
    bool finite = true;
    for (size_t i = 0; i < taps.size(); i++) finite = finite && std::isfinite(float(taps[i]));
    if (rest != 1 || D < 1 || D > M || taps.empty() || taps.size() > 64 * M || !finite) {
      ConfigError err;
      err << "Can not configure " << Grid::name() << " node: M = " << M << Grid::ruleM() << ", D = " << D << " (1 ... M), "
          << taps.size() << " taps (1 ... 64 M, all finite as floats)";
      throw err;
    }
    const size_t K = _K;
    if (_sel.empty()) for (size_t k = 0; k < K; k++) _sel.push_back(int(k));
    std::vector<bool> seen(K, false);
    for (size_t i = 0; i < _sel.size(); i++) {
      if (_sel[i] < 0 || size_t(_sel[i]) >= K || seen[size_t(_sel[i])]) {
        ConfigError err;
        err << "Can not configure " << Grid::name() << " node: channel " << _sel[i] << " (row " << i << ") is outside [0, " << K << ") or selected twice";
        throw err;
      }
      seen[size_t(_sel[i])] = true;
    }
    if (_modes.empty()) _modes.assign(_sel.size(), int(SDRHIP_EPI_FM));
    if (_gains.empty()) _gains.assign(_sel.size(), 1.0f);
    bool ok = _modes.size() == _sel.size() && _gains.size() == _sel.size();
    for (size_t i = 0; ok && i < _sel.size(); i++)
      ok = (_modes[i] == SDRHIP_EPI_FM || _modes[i] == SDRHIP_EPI_AM || _modes[i] == SDRHIP_EPI_USB) && std::isfinite(_gains[i]);
    if (!ok) {
      ConfigError err;
      err << "Can not configure " << Grid::name() << " node: " << _modes.size() << " modes and " << _gains.size() << " gains for " << _sel.size()
          << " rows (one each; SDRHIP_EPI_FM, _AM or _USB; finite gains)";
      throw err;
    }
    for (size_t i = 0; i < _sel.size(); i++) _outs.push_back(new Out());
  }
  virtual ~AudioChannelizerNode() {
    _release();
    for (size_t i = 0; i < _outs.size(); i++) delete _outs[i];
  }

  /** The rows delivered, and the channel row i holds. */
  size_t rows() const { return _sel.size(); }
  int channel(size_t i) const { return _sel[i]; }
  int mode(size_t i) const { return _modes[i]; }
  float gain(size_t i) const { return _gains[i]; }
  Source *source(size_t i) { return _outs[i]; }
  sdrhip_ctx *context() const { return _ctx; }
  /** The smallest row stride of processDev: the most outputs a buffer of the configured size gives. */
  size_t outStride() const { return _outStride; }

  virtual void config(const Config &cfg) {
    if (!cfg.hasType() || !cfg.hasSampleRate() || !cfg.hasBufferSize()) return;
    detail::checkType<In>(cfg, (std::string(Grid::name()) + " node").c_str());
    _release();
    _bs = cfg.bufferSize();
    if (_bs == 0) return;
    _ctx = Device::get(_device);
    std::vector<int> modes(_K, int(SDRHIP_EPI_FM));   // per channel: the rows' own, FM and 1 elsewhere
    std::vector<float> gains(_K, 1.0f);
    for (size_t i = 0; i < _sel.size(); i++) { modes[size_t(_sel[i])] = _modes[i]; gains[size_t(_sel[i])] = _gains[i]; }
    detail::configCheck(Grid::create(_ctx, int(_M), int(_D), _taps.data(), int(_taps.size()), _bs, modes.data(), gains.data(), _plan.out()),
                        Grid::name());
    detail::configCheck(sdrhip_chanaudio_set_channels(_plan, _sel.data(), int(_sel.size())), Grid::name());
    _outStride = (_bs + _D - 1) / _D;
    const size_t R = _sel.size();
    _din.alloc(_ctx, _bs * sizeof(In), Grid::name());
    _dout.alloc(_ctx, R * _outStride * sizeof(int16_t), Grid::name());
    _stageOut = Buffer<int16_t>(R * _outStride);
    _pinOut.reset(_stageOut.data(), R * _outStride * sizeof(int16_t), Grid::name());
    for (size_t i = 0; i < R; i++) _outs[i]->configure(Config(Config::typeId<int16_t>(), cfg.sampleRate() / double(_D), _outStride, 1));
  }

  virtual void process(const Buffer<In> &b, bool) {
    if (!_plan || b.size() > _bs || b.size() == 0) return;
    // the per-row outputs are views of _stageOut: while a consumer still holds one of the last round, this round is dropped
    if (!_stageOut.isUnused()) {
      LogMessage msg(LOG_WARNING);
      msg << _gpuName << ": output of the last round still in use downstream; buffer dropped";
      Logger::get().log(msg);
      return;
    }
    const size_t R = _sel.size();
    size_t n = 0;
    if (!detail::processOk(sdrhip_memcpy_h2d_async(_ctx, _din.get(), b.data(), b.size() * sizeof(In)), _gpuName.c_str()) ||
        !detail::processOk(sdrhip_chanaudio_process_dev(_plan, _din.get(), b.size(), _dout.get(), _outStride, &n), _gpuName.c_str()) ||
        !detail::processOk(sdrhip_memcpy_d2h_async(_ctx, _stageOut.data(), _dout.get(), R * _outStride * sizeof(int16_t)), _gpuName.c_str()) ||
        !detail::processOk(sdrhip_ctx_synchronize(_ctx), _gpuName.c_str()))
      return;
    if (n == 0) return;
    for (size_t i = 0; i < R; i++) _outs[i]->emit(_stageOut.sub(i * _outStride, n), false);
  }

  /** One row of n device samples in, rows() device rows out (outStride in int16 elements, at least the call's output count);
   * one launch on the context's stream, nothing is synchronised. After config() only. */
  bool processDev(const void *inDev, size_t n, void *outDev, size_t outStride, size_t *nOut) {
    return detail::processOk(sdrhip_chanaudio_process_dev(_plan, inDev, n, outDev, outStride, nOut), _gpuName.c_str());
  }
  /** A new prototype of the same length; the stream goes on. */
  void setTaps(const std::vector<double> &taps) {
    if (taps.size() != _taps.size()) {
      ConfigError err;
      err << Grid::name() << ": " << taps.size() << " taps where the node has " << _taps.size();
      throw err;
    }
    if (_plan) detail::configCheck(sdrhip_chanaudio_set_taps(_plan, taps.data()), Grid::name());
    _taps = taps;
  }
  /** Row i's demodulator from now on (the row starts from last = 0) / its gain; before config() they are only noted. */
  void setMode(size_t i, int mode) {
    if (_plan) detail::configCheck(sdrhip_chanaudio_set_mode(_plan, int(i), mode), Grid::name());
    _modes.at(i) = mode;
  }
  void setGain(size_t i, float gain) {
    if (_plan) detail::configCheck(sdrhip_chanaudio_set_gain(_plan, int(i), gain), Grid::name());
    _gains.at(i) = gain;
  }
  void reset() { if (_plan) detail::configCheck(sdrhip_chanaudio_reset(_plan), Grid::name()); }
  /** The samples taken since config() or reset(). */
  uint64_t consumed() const {
    uint64_t c = 0;
    if (_plan) detail::configCheck(sdrhip_chanaudio_get_state(_plan, &c, 0, 0, 0, 0), Grid::name());
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

  size_t _M, _K, _D;        // _K: the grid's channels
  std::vector<double> _taps;
  std::vector<int> _sel, _modes;
  std::vector<float> _gains;
  int _device;
  sdrhip_ctx *_ctx;
  detail::Handle<sdrhip_chanaudio, sdrhip_chanaudio_destroy> _plan;
  detail::DeviceMem _din, _dout;
  detail::Pinned _pinOut;   // the registration of _stageOut
  size_t _bs, _outStride;
  std::vector<Out *> _outs;
  Buffer<int16_t> _stageOut;
  std::string _gpuName;     // "gpu::<name>", for the log
};

template <class Scalar>
class AudioChannelizer : public AudioChannelizerNode< detail::ComplexAudioGrid<Scalar> > {
public:
  /** M channels decimated by D with the prototype low-pass `taps`; channels: the channels to deliver, any order, no duplicates
   * (empty: all M in order); modes[i], gains[i]: row i's demodulator (SDRHIP_EPI_FM, _AM or _USB) and gain (empty: FM, 1). The
   * rules of sdrhip_chanaudio_create are checked here and throw ConfigError: 2 <= M <= 4096 with prime factors up to 13,
   * 1 <= D <= M, 1 <= taps.size() <= 64 M, every tap finite as a float, every channel in [0, M), once, a mode and a gain per row,
   * every mode one of the three, every gain finite. */
  AudioChannelizer(size_t M, size_t D, const std::vector<double> &taps, const std::vector<int> &channels = std::vector<int>(),
                   const std::vector<int> &modes = std::vector<int>(), const std::vector<float> &gains = std::vector<float>(), int device = 0)
    : AudioChannelizerNode< detail::ComplexAudioGrid<Scalar> >(M, D, taps, channels, modes, gains, device) {}
};

}  // namespace gpu
}  // namespace sdr
#endif
