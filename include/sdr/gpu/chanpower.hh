/* sdr/gpu/chanpower.hh — gpu::ChannelPower<Scalar>: the channel power monitor (sdrhip_chanpower_*, include/sdrhip_chanpower.h has
 * the contract) as a graph node: a Sink of std::complex<Scalar> — ONE antenna stream, the one a gpu::Channelizer or
 * gpu::AudioChannelizer beside it takes — that stores no rows. Per buffer it keeps the M sums of |y_k|^2, per channel a smoothed
 * level and an open / closed flag with hysteresis; occupied() is the ascending channel list the channelizers' constructors and
 * set_channels take. Scalar is int16_t or float. The node has no reference node behind it.
 *
 * Per buffer: one H2D copy, two launches, one D2H copy of M doubles. processDev() runs the same plan on a device row of the node's
 * device and synchronises nothing.
 *
 * The node's body is gpu::ChannelPowerNode<Grid> on detail::ChannelNodeBase (channelizer.hh), which has the M / D / taps rule,
 * setTaps, reset and consumed: Grid says what the complex node and the real-input one of chanreal.hh
 * (gpu::RealChannelPower<Scalar>) differ in; channels() is the grid's channel count.
 */
#ifndef SDR_GPU_CHANPOWER_HH
#define SDR_GPU_CHANPOWER_HH

#include "channelizer.hh"
#include "../../sdrhip_chanpower.h"

#include <cmath>
#include <sstream>
#include <string>
#include <vector>

namespace sdr {
namespace gpu {

namespace detail {
/** What the node bodies call of sdrhip_chanpower.h (no rows: no selection, and process_dev has its own shape). */
struct ChanPowerApi {
  typedef sdrhip_chanpower Plan;
  static int destroy(Plan *p) { return sdrhip_chanpower_destroy(p); }
  static int setTaps(Plan *p, const double *taps) { return sdrhip_chanpower_set_taps(p, taps); }
  static int reset(Plan *p) { return sdrhip_chanpower_reset(p); }
  static int consumed(Plan *p, uint64_t *c) { return sdrhip_chanpower_get_state(p, c, 0, 0, 0); }
};

/** The alpha clause of the monitor's rule message. */
inline std::string alphaClause(double alpha) {
  std::ostringstream s;
  s << ", alpha = " << alpha << " (in (0, 1])";
  return s.str();
}

/** The complex monitor's grid: detail::ComplexGrid with sdrhip_chanpower_create. */
template <class Scalar> struct ComplexPowerGrid : ComplexGrid<Scalar> {
  typedef ChanPowerApi Api;
  static const char *name() { return "ChannelPower"; }
  static int create(sdrhip_ctx *ctx, int M, int D, const double *taps, int nTaps, size_t maxIn, double alpha, sdrhip_chanpower **out) {
    return sdrhip_chanpower_create(ctx, ChannelizerType<Scalar>::dtype, M, D, taps, nTaps, maxIn, alpha, out);
  }
};
}  // namespace detail

template <class Grid>
class ChannelPowerNode : public detail::ChannelNodeBase<Grid> {
public:
  typedef typename Grid::In In;

  /** M, D, taps and alpha as gpu::ChannelPower and gpu::RealChannelPower say; the grid's rules are checked here and throw
   * ConfigError. */
  ChannelPowerNode(size_t M, size_t D, const std::vector<double> &taps, double alpha, int device)
    : detail::ChannelNodeBase<Grid>(M, D, taps, device, alpha > 0.0 && alpha <= 1.0, detail::alphaClause(alpha)), _alpha(alpha), _last(0) {
    _open.assign(_K, HUGE_VAL);
    _close.assign(_K, 0.0);
    _sums.assign(_K, 0.0);
  }
  virtual ~ChannelPowerNode() { _release(); }

  size_t channels() const { return _K; }

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
  virtual void config(const Config &cfg) {
    if (!this->_begin(cfg)) return;
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
  /** The buffers that completed an output since config() or reset(). */
  uint64_t calls() const {
    uint64_t c = 0;
    if (_plan) detail::configCheck(sdrhip_chanpower_get_state(_plan, 0, 0, 0, &c), Grid::name());
    return c;
  }

protected:
  virtual void _release() {
    detail::ChannelNodeBase<Grid>::_release();
    _dsum.reset();
  }

  using detail::ChannelNodeBase<Grid>::_M;
  using detail::ChannelNodeBase<Grid>::_K;
  using detail::ChannelNodeBase<Grid>::_D;
  using detail::ChannelNodeBase<Grid>::_taps;
  using detail::ChannelNodeBase<Grid>::_ctx;
  using detail::ChannelNodeBase<Grid>::_plan;
  using detail::ChannelNodeBase<Grid>::_din;
  using detail::ChannelNodeBase<Grid>::_bs;
  using detail::ChannelNodeBase<Grid>::_gpuName;
  std::vector<double> _open, _close, _sums;
  double _alpha;
  detail::DeviceMem _dsum;
  size_t _last;
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
