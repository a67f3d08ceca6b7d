/* sdr/gpu/chanpower.hh — gpu::ChannelPower<Scalar>: the channel power monitor (sdrhip_chanpower_*, include/sdrhip_chanpower.h has
 * the contract) as a graph node: a Sink of std::complex<Scalar> — ONE antenna stream, the one a gpu::Channelizer or
 * gpu::AudioChannelizer beside it takes — that stores no rows. Per buffer it keeps the M sums of |y_k|^2, per channel a smoothed
 * level and an open / closed flag with hysteresis; occupied() is the ascending channel list the channelizers' constructors and
 * set_channels take. Scalar is int16_t or float. The node has no reference node behind it.
 *
 * Per buffer: one H2D copy, two launches, one D2H copy of M doubles. processDev() runs the same plan on a device row of the node's
 * device and synchronises nothing.
 *
 * The node's body is gpu::ChannelPowerNode<Grid>, as gpu::ChannelizerNode is gpu::Channelizer's: Grid says what the complex node
 * and the real-input one of chanreal.hh (gpu::RealChannelPower<Scalar>) differ in; channels() is the grid's channel count.
 */
#ifndef SDR_GPU_CHANPOWER_HH
#define SDR_GPU_CHANPOWER_HH

#include "channelizer.hh"
#include "../../sdrhip_chanpower.h"

#include <cmath>
#include <string>
#include <vector>

namespace sdr {
namespace gpu {

namespace detail {
/** The complex monitor's grid: detail::ComplexGrid with sdrhip_chanpower_create. */
template <class Scalar> struct ComplexPowerGrid : ComplexGrid<Scalar> {
  static const char *name() { return "ChannelPower"; }
  static int create(sdrhip_ctx *ctx, int M, int D, const double *taps, int nTaps, size_t maxIn, double alpha, sdrhip_chanpower **out) {
    return sdrhip_chanpower_create(ctx, ChannelizerType<Scalar>::dtype, M, D, taps, nTaps, maxIn, alpha, out);
  }
};
}  // namespace detail

template <class Grid>
class ChannelPowerNode : public Sink<typename Grid::In> {
public:
  typedef typename Grid::In In;

  /** M, D, taps and alpha as gpu::ChannelPower and gpu::RealChannelPower say; the grid's rules are checked here and throw
   * ConfigError. */
  ChannelPowerNode(size_t M, size_t D, const std::vector<double> &taps, double alpha, int device)
    : Sink<In>(), _M(M), _K(Grid::admitsM(M) ? Grid::channels(M) : 0), _D(D), _taps(taps), _alpha(alpha), _device(device), _ctx(0), _bs(0),
      _last(0), _gpuName(std::string("gpu::") + Grid::name()) {
    size_t rest = Grid::admitsM(M) ? Grid::transform(M) : 0;
    const size_t primes[] = {2, 3, 5, 7, 11, 13};
    for (size_t q = 0; q < 6; q++) while (rest > 1 && rest % primes[q] == 0) rest /= primes[q];
    bool finite = true;
    for (size_t i = 0; i < taps.size(); i++) finite = finite && std::isfinite(float(taps[i]));
    if (rest != 1 || D < 1 || D > M || taps.empty() || taps.size() > 64 * M || !finite || !(alpha > 0.0 && alpha <= 1.0)) {
      ConfigError err;
      err << "Can not configure " << Grid::name() << " node: M = " << M << Grid::ruleM() << ", D = " << D << " (1 ... M), "
          << taps.size() << " taps (1 ... 64 M, all finite as floats), alpha = " << alpha << " (in (0, 1])";
      throw err;
    }
    _open.assign(_K, HUGE_VAL);
    _close.assign(_K, 0.0);
    _sums.assign(_K, 0.0);
  }
  virtual ~ChannelPowerNode() { _release(); }

  size_t channels() const { return _K; }
  sdrhip_ctx *context() const { return _ctx; }

  /** Absolute thresholds in the units of |y|^2, for every channel or per channel: 0 <= close <= open, no NaN (ConfigError). They
   * hold from the next buffer on, and over config(). */
  void setThresholds(double open, double close) { setThresholds(std::vector<double>(_K, open), std::vector<double>(_K, close)); }
  void setThresholds(const std::vector<double> &open, const std::vector<double> &close) {
    bool ok = open.size() == _K && close.size() == _K;
    for (size_t k = 0; ok && k < _K; k++) ok = close[k] >= 0.0 && close[k] <= open[k];
    if (!ok) {
      ConfigError err;
      err << Grid::name() << ": thresholds want " << _K << " values each with 0 <= close <= open";
      throw err;
    }
    if (_plan) detail::configCheck(sdrhip_chanpower_set_thresholds(_plan, open.data(), close.data()), Grid::name());
    _open = open;
    _close = close;
  }
  void setAlpha(double alpha) {
    if (!(alpha > 0.0 && alpha <= 1.0)) {
      ConfigError err;
      err << Grid::name() << ": alpha = " << alpha << " outside (0, 1]";
      throw err;
    }
    if (_plan) detail::configCheck(sdrhip_chanpower_set_alpha(_plan, alpha), Grid::name());
    _alpha = alpha;
  }
  /** A new prototype of the same length; the stream, the levels and the flags go on. */
  void setTaps(const std::vector<double> &taps) {
    if (taps.size() != _taps.size()) {
      ConfigError err;
      err << Grid::name() << ": " << taps.size() << " taps where the node has " << _taps.size();
      throw err;
    }
    if (_plan) detail::configCheck(sdrhip_chanpower_set_taps(_plan, taps.data()), Grid::name());
    _taps = taps;
  }

  virtual void config(const Config &cfg) {
    if (!cfg.hasType() || !cfg.hasSampleRate() || !cfg.hasBufferSize()) return;
    detail::checkType<In>(cfg, (std::string(Grid::name()) + " node").c_str());
    _release();
    _bs = cfg.bufferSize();
    if (_bs == 0) return;
    _ctx = Device::get(_device);
    detail::configCheck(Grid::create(_ctx, int(_M), int(_D), _taps.data(), int(_taps.size()), _bs, _alpha, _plan.out()), Grid::name());
    detail::configCheck(sdrhip_chanpower_set_thresholds(_plan, _open.data(), _close.data()), Grid::name());
    _din.alloc(_ctx, _bs * sizeof(In), Grid::name());
    _dsum.alloc(_ctx, _K * sizeof(double), Grid::name());
  }

  virtual void process(const Buffer<In> &b, bool) {
    if (!_plan || b.size() > _bs || b.size() == 0) return;
    size_t n = 0;
    if (!detail::processOk(sdrhip_memcpy_h2d_async(_ctx, _din.get(), b.data(), b.size() * sizeof(In)), _gpuName.c_str()) ||
        !detail::processOk(sdrhip_chanpower_process_dev(_plan, _din.get(), b.size(), _dsum.template as<double>(), &n), _gpuName.c_str()) ||
        !detail::processOk(sdrhip_memcpy_d2h(_ctx, _sums.data(), _dsum.get(), _K * sizeof(double)), _gpuName.c_str()))
      return;
    _last = n;
  }

  /** One row of n device samples in; sumDev: channels() doubles on the device, or 0 where only the levels and flags are wanted. Two launches
   * on the context's stream, nothing is synchronised. After config() only. */
  bool processDev(const void *inDev, size_t n, double *sumDev, size_t *nOut) {
    return detail::processOk(sdrhip_chanpower_process_dev(_plan, inDev, n, sumDev, nOut), _gpuName.c_str());
  }

  /** The last buffer's sums of |y_k|^2 and the outputs per channel they were taken over. */
  const std::vector<double> &sums() const { return _sums; }
  size_t lastCount() const { return _last; }
  /** level[k] and open[k] of every channel behind the buffers taken so far (zeros before config()). */
  std::vector<double> levels() const {
    std::vector<double> v(_K, 0.0);
    if (_plan) detail::configCheck(sdrhip_chanpower_get_levels(_plan, v.data(), 0, int(_K)), Grid::name());
    return v;
  }
  std::vector<bool> open() const {
    std::vector<unsigned char> f(_K, 0);
    if (_plan) detail::configCheck(sdrhip_chanpower_get_levels(_plan, 0, f.data(), int(_K)), Grid::name());
    return std::vector<bool>(f.begin(), f.end());
  }
  /** The open channels, ascending: what the channelizers take as their selection (where it is not empty). */
  std::vector<int> occupied() const {
    std::vector<int> idx(_K, 0);
    int count = 0;
    if (_plan) detail::configCheck(sdrhip_chanpower_get_occupied(_plan, idx.data(), int(_K), &count), Grid::name());
    idx.resize(size_t(count));
    return idx;
  }
  /** As freshly configured, with the current taps, alpha and thresholds. */
  void reset() { if (_plan) detail::configCheck(sdrhip_chanpower_reset(_plan), Grid::name()); }
  /** The samples taken, and the buffers that completed an output, since config() or reset(). */
  uint64_t consumed() const {
    uint64_t c = 0;
    if (_plan) detail::configCheck(sdrhip_chanpower_get_state(_plan, &c, 0, 0, 0), Grid::name());
    return c;
  }
  uint64_t calls() const {
    uint64_t c = 0;
    if (_plan) detail::configCheck(sdrhip_chanpower_get_state(_plan, 0, 0, 0, &c), Grid::name());
    return c;
  }

protected:
  /** In this order: the device is idle before anything it may still use goes. */
  void _release() {
    if (_ctx) sdrhip_ctx_synchronize(_ctx);
    _plan.reset();
    _din.reset();
    _dsum.reset();
  }

  size_t _M, _K, _D;        // _K: the grid's channels
  std::vector<double> _taps, _open, _close, _sums;
  double _alpha;
  int _device;
  sdrhip_ctx *_ctx;
  detail::Handle<sdrhip_chanpower, sdrhip_chanpower_destroy> _plan;
  detail::DeviceMem _din, _dsum;
  size_t _bs, _last;
  std::string _gpuName;     // "gpu::<name>", for the log
};

template <class Scalar>
class ChannelPower : public ChannelPowerNode< detail::ComplexPowerGrid<Scalar> > {
public:
  /** M channels decimated by D with the prototype low-pass `taps`, the level following the buffers' means with the factor alpha.
   * The rules of sdrhip_chanpower_create are checked here and throw ConfigError: 2 <= M <= 4096 with prime factors up to 13,
   * 1 <= D <= M, 1 <= taps.size() <= 64 M, every tap finite as a float, 0 < alpha <= 1. */
  ChannelPower(size_t M, size_t D, const std::vector<double> &taps, double alpha = 0.25, int device = 0)
    : ChannelPowerNode< detail::ComplexPowerGrid<Scalar> >(M, D, taps, alpha, device) {}
};

}  // namespace gpu
}  // namespace sdr
#endif
