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
 *
 * The family's node bodies live here. Grid says what the complex nodes and the real-input ones of chanreal.hh differ in (the
 * input element, the rule for M, the channel count, the create call) and names the Api of its C header: the handle type and the C
 * calls a body uses. detail::ChannelNodeBase<Grid> holds what every node of the family has (the M / D / taps rule, the plan,
 * setTaps, reset, consumed); detail::RowNode<Grid, Elem> on top of it is the row-emitting node — gpu::ChannelizerNode<Grid> here,
 * gpu::AudioChannelizerNode<Grid> in chanaudio.hh with modes and gains added; gpu::ChannelPowerNode<Grid> (chanpower.hh) sits on
 * the base directly.
 */
#ifndef SDR_GPU_CHANNELIZER_HH
#define SDR_GPU_CHANNELIZER_HH

#include "nodes.hh"
#include "../../sdrhip_channelizer.h"

#include <cmath>
#include <sstream>
#include <string>
#include <vector>

namespace sdr {
namespace gpu {

namespace detail {
template <class Scalar> struct ChannelizerType;
template <> struct ChannelizerType<int16_t> { enum { dtype = SDRHIP_CHAN_CS16 }; };
template <> struct ChannelizerType<float> { enum { dtype = SDRHIP_CHAN_CF32 }; };

/** What the node bodies call of sdrhip_channelizer.h; chanaudio.hh and chanpower.hh have their headers' (the monitor's has no
 * row calls). */
struct ChannelizerApi {
  typedef sdrhip_channelizer Plan;
  static int destroy(Plan *p) { return sdrhip_channelizer_destroy(p); }
  static int setChannels(Plan *p, const int *idx, int n) { return sdrhip_channelizer_set_channels(p, idx, n); }
  static int processDev(Plan *p, const void *in, size_t n, void *out, size_t stride, size_t *nOut) {
    return sdrhip_channelizer_process_dev(p, in, n, out, stride, nOut);
  }
  static int setTaps(Plan *p, const double *taps) { return sdrhip_channelizer_set_taps(p, taps); }
  static int reset(Plan *p) { return sdrhip_channelizer_reset(p); }
  static int consumed(Plan *p, uint64_t *c) { return sdrhip_channelizer_get_state(p, c, 0, 0); }
};

/** The complex node's grid: M channels of an M-point transform, sdrhip_channelizer_create. */
template <class Scalar> struct ComplexGrid {
  typedef std::complex<Scalar> In;
  typedef ChannelizerApi Api;
  static const char *name() { return "Channelizer"; }
  static const char *ruleM() { return " (2 ... 4096, prime factors up to 13)"; }
  static bool admitsM(size_t M) { return M >= 2 && M <= 4096; }
  static size_t transform(size_t M) { return M; }
  static size_t channels(size_t M) { return M; }
  static int create(sdrhip_ctx *ctx, int M, int D, const double *taps, int nTaps, size_t maxIn, sdrhip_channelizer **out) {
    return sdrhip_channelizer_create(ctx, ChannelizerType<Scalar>::dtype, M, D, taps, nTaps, maxIn, out);
  }
};

/** The grid's rules for M, D and the taps; ConfigError. own, suffix: a node's own rule checked with them (false: broken) and its
 * clause of the message. */
template <class Grid>
inline void checkGrid(size_t M, size_t D, const std::vector<double> &taps, bool own = true, const std::string &suffix = std::string()) {
  size_t rest = Grid::admitsM(M) ? Grid::transform(M) : 0;
  const size_t primes[] = {2, 3, 5, 7, 11, 13};
  for (size_t q = 0; q < 6; q++) while (rest > 1 && rest % primes[q] == 0) rest /= primes[q];
  bool finite = true;
  for (size_t i = 0; i < taps.size(); i++) finite = finite && std::isfinite(float(taps[i]));
  if (rest != 1 || D < 1 || D > M || taps.empty() || taps.size() > 64 * M || !finite || !own) {
    ConfigError err;
    err << "Can not configure " << Grid::name() << " node: M = " << M << Grid::ruleM() << ", D = " << D << " (1 ... M), "
        << taps.size() << " taps (1 ... 64 M, all finite as floats)" << suffix;
    throw err;
  }
}

/** The selection rule: every channel in [0, K), once; an empty selection becomes all K in order. ConfigError. */
template <class Grid>
inline void checkSelection(std::vector<int> &sel, size_t K) {
  if (sel.empty()) for (size_t k = 0; k < K; k++) sel.push_back(int(k));
  std::vector<bool> seen(K, false);
  for (size_t i = 0; i < sel.size(); i++) {
    if (sel[i] < 0 || size_t(sel[i]) >= K || seen[size_t(sel[i])]) {
      ConfigError err;
      err << "Can not configure " << Grid::name() << " node: channel " << sel[i] << " (row " << i << ") is outside [0, " << K << ") or selected twice";
      throw err;
    }
    seen[size_t(sel[i])] = true;
  }
}

/** What every node of the family is: a Sink of the grid's input element with the grid's rules checked, a plan of the grid's Api
 * and the device row a buffer is copied to. */
template <class Grid>
class ChannelNodeBase : public Sink<typename Grid::In> {
public:
  typedef typename Grid::In In;
  typedef typename Grid::Api Api;

  sdrhip_ctx *context() const { return _ctx; }
  /** The node's plan handle (null before config()): what gpu::ChannelGroup borrows. The node stays its owner. */
  typename Api::Plan *plan() const { return _plan.get(); }
  /** A new prototype of the same length; the stream (and a monitor's levels and flags) go on. */
  void setTaps(const std::vector<double> &taps) {
    if (taps.size() != _taps.size()) {
      ConfigError err;
      err << Grid::name() << ": " << taps.size() << " taps where the node has " << _taps.size();
      throw err;
    }
    if (_plan) configCheck(Api::setTaps(_plan, taps.data()), Grid::name());
    _taps = taps;
  }
  /** As freshly configured, with the current parameters. */
  void reset() { if (_plan) configCheck(Api::reset(_plan), Grid::name()); }
  /** The samples taken since config() or reset(). */
  uint64_t consumed() const {
    uint64_t c = 0;
    if (_plan) configCheck(Api::consumed(_plan, &c), Grid::name());
    return c;
  }

protected:
  ChannelNodeBase(size_t M, size_t D, const std::vector<double> &taps, int device, bool own = true, const std::string &suffix = std::string())
    : Sink<In>(), _M(M), _K(Grid::admitsM(M) ? Grid::channels(M) : 0), _D(D), _taps(taps), _device(device), _ctx(0), _bs(0),
      _gpuName(std::string("gpu::") + Grid::name()) {
    checkGrid<Grid>(M, D, taps, own, suffix);
  }
  /** The head of config(): false where there is nothing to configure (yet); else the old plan is gone, _bs and _ctx are set. */
  bool _begin(const Config &cfg) {
    if (!cfg.hasType() || !cfg.hasSampleRate() || !cfg.hasBufferSize()) return false;
    checkType<In>(cfg, (std::string(Grid::name()) + " node").c_str());
    _release();
    _bs = cfg.bufferSize();
    if (_bs == 0) return false;
    _ctx = Device::get(_device);
    return true;
  }
  /** In this order: the device is idle before anything it may still use goes; a node's own buffers follow. */
  virtual void _release() {
    if (_ctx) sdrhip_ctx_synchronize(_ctx);
    _plan.reset();
    _din.reset();
  }

  size_t _M, _K, _D;        // _K: the grid's channels
  std::vector<double> _taps;
  int _device;
  sdrhip_ctx *_ctx;
  Handle<typename Api::Plan, Api::destroy> _plan;
  DeviceMem _din;
  size_t _bs;
  std::string _gpuName;     // "gpu::<name>", for the log
};

/** The row-emitting node: one Source per selected channel, each emitting Buffer<Elem>. A subclass creates the plan. */
template <class Grid, class Elem>
class RowNode : public ChannelNodeBase<Grid> {
public:
  typedef typename Grid::In In;
  typedef typename Grid::Api Api;
  typedef ChannelBank<int16_t>::Out Out;

  virtual ~RowNode() {
    _release();
    for (size_t i = 0; i < _outs.size(); i++) delete _outs[i];
  }

  /** The rows delivered, and the channel row i holds. */
  size_t rows() const { return _sel.size(); }
  int channel(size_t i) const { return _sel[i]; }
  Source *source(size_t i) { return _outs[i]; }
  /** The smallest row stride of processDev: the most outputs a buffer of the configured size gives. */
  size_t outStride() const { return _outStride; }

  virtual void config(const Config &cfg) {
    if (!this->_begin(cfg)) return;
    configCheck(_create(), Grid::name());
    configCheck(Api::setChannels(_plan, _sel.data(), int(_sel.size())), Grid::name());
    _outStride = (_bs + _D - 1) / _D;
    const size_t R = _sel.size();
    _din.alloc(_ctx, _bs * sizeof(In), Grid::name());
    _dout.alloc(_ctx, R * _outStride * sizeof(Elem), Grid::name());
    _stageOut = Buffer<Elem>(R * _outStride);
    _pinOut.reset(_stageOut.data(), R * _outStride * sizeof(Elem), Grid::name());
    for (size_t i = 0; i < R; i++) _outs[i]->configure(Config(Config::typeId<Elem>(), cfg.sampleRate() / double(_D), _outStride, 1));
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
    if (!processOk(sdrhip_memcpy_h2d_async(_ctx, _din.get(), b.data(), b.size() * sizeof(In)), _gpuName.c_str()) ||
        !processOk(Api::processDev(_plan, _din.get(), b.size(), _dout.get(), _outStride, &n), _gpuName.c_str()) ||
        !processOk(sdrhip_memcpy_d2h_async(_ctx, _stageOut.data(), _dout.get(), R * _outStride * sizeof(Elem)), _gpuName.c_str()) ||
        !processOk(sdrhip_ctx_synchronize(_ctx), _gpuName.c_str()))
      return;
    if (n == 0) return;
    for (size_t i = 0; i < R; i++) _outs[i]->emit(_stageOut.sub(i * _outStride, n), false);
  }

  /** One row of n device samples in, rows() device rows out (outStride in elements of the rows, at least the call's output
   * count); one launch on the context's stream, nothing is synchronised. After config() only. */
  bool processDev(const void *inDev, size_t n, void *outDev, size_t outStride, size_t *nOut) {
    return processOk(Api::processDev(_plan, inDev, n, outDev, outStride, nOut), _gpuName.c_str());
  }

protected:
  RowNode(size_t M, size_t D, const std::vector<double> &taps, const std::vector<int> &channels, int device)
    : ChannelNodeBase<Grid>(M, D, taps, device), _sel(channels), _outStride(0) {
    checkSelection<Grid>(_sel, _K);
  }
  /** Once the subclass's own rules have passed. */
  void _makeOuts() { for (size_t i = 0; i < _sel.size(); i++) _outs.push_back(new Out()); }
  /** The grid's create call into _plan.out(), for buffers of _bs samples on _ctx. */
  virtual int _create() = 0;
  virtual void _release() {
    ChannelNodeBase<Grid>::_release();
    _dout.reset();
    _pinOut.reset();
    _stageOut.unref();
  }

  using ChannelNodeBase<Grid>::_M;
  using ChannelNodeBase<Grid>::_K;
  using ChannelNodeBase<Grid>::_D;
  using ChannelNodeBase<Grid>::_taps;
  using ChannelNodeBase<Grid>::_ctx;
  using ChannelNodeBase<Grid>::_plan;
  using ChannelNodeBase<Grid>::_din;
  using ChannelNodeBase<Grid>::_bs;
  using ChannelNodeBase<Grid>::_gpuName;
  std::vector<int> _sel;
  DeviceMem _dout;
  Pinned _pinOut;           // the registration of _stageOut
  size_t _outStride;
  std::vector<Out *> _outs;
  Buffer<Elem> _stageOut;
};
}  // namespace detail

template <class Grid>
class ChannelizerNode : public detail::RowNode<Grid, cf32> {
public:
  /** M, D, taps and channels as gpu::Channelizer and gpu::RealChannelizer say; the grid's rules are checked here and throw
   * ConfigError. */
  ChannelizerNode(size_t M, size_t D, const std::vector<double> &taps, const std::vector<int> &channels, int device)
    : detail::RowNode<Grid, cf32>(M, D, taps, channels, device) { this->_makeOuts(); }

protected:
  virtual int _create() {
    return Grid::create(this->_ctx, int(this->_M), int(this->_D), this->_taps.data(), int(this->_taps.size()), this->_bs, this->_plan.out());
  }
};

template <class Scalar>
class Channelizer : public ChannelizerNode< detail::ComplexGrid<Scalar> > {
public:
  /** M channels decimated by D with the prototype low-pass `taps`; channels: the channels to deliver, any order, no duplicates
   * (empty: all M in order). The rules of sdrhip_channelizer_create are checked here and throw ConfigError: 2 <= M <= 4096 with
   * prime factors up to 13, 1 <= D <= M, 1 <= taps.size() <= 64 M, every tap finite as a float, every channel in [0, M), once. */
  Channelizer(size_t M, size_t D, const std::vector<double> &taps, const std::vector<int> &channels = std::vector<int>(), int device = 0)
    : ChannelizerNode< detail::ComplexGrid<Scalar> >(M, D, taps, channels, device) {}
};

}  // namespace gpu
}  // namespace sdr
#endif
