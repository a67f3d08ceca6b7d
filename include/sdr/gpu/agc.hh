/* sdr/gpu/agc.hh — gpu::AGC<Scalar>, the drop-in for the reference's AGC<int16_t> / AGC<float> (src/utils.hh:658-793), and
 * gpu::AGCBank<Scalar>, N such nodes over rows in one launch (sdrhip_agc_*, include/sdrhip_agc.h).
 *
 * One deviation from the reference: AGC::process sends its whole output buffer whatever the input's length, so the samples
 * behind a short buffer are stale. gpu::AGC sends head(n), the n samples of the buffer it was given.
 */
#ifndef SDR_GPU_AGC_HH
#define SDR_GPU_AGC_HH

#include "nodes.hh"
#include "../../sdrhip_agc.h"

namespace sdr {
namespace gpu {

namespace detail {
template <class Scalar> struct AgcType;
template <> struct AgcType<int16_t> { enum { dtype = SDRHIP_AGC_I16 }; };
template <> struct AgcType<float> { enum { dtype = SDRHIP_AGC_F32 }; };
inline float agcLambda(double tau, double Fs, const char *what) {
  float l = 0;
  configCheck(sdrhip_design_agc_lambda(tau, Fs, &l), what);
  return l;
}
inline float agcTarget(int dtype, double target, const char *what) {
  float t = float(target);
  if (0 == target) configCheck(sdrhip_design_agc_target(dtype, &t), what);
  return t;
}
}  // namespace detail

/** AGC<Scalar>(tau, target) with the reference's surface. Before the first config() the setters are remembered; afterwards they
 * act on the device node, and gain() reads it back. */
template <class Scalar>
class AGC : public Sink<Scalar>, public Source {
public:
  AGC(double tau = 0.1, double target = 0, int device = 0)
    : _enabled(true), _tau(float(tau)), _target(detail::agcTarget(detail::AgcType<Scalar>::dtype, target, "AGC")), _gain(1),
      _sampleRate(0), _device(device) {}
  virtual ~AGC() { _buffer.unref(); }

  inline bool enabled() const { return _enabled; }
  inline void enable(bool enabled) {
    _enabled = enabled;
    if (_plan) detail::configCheck(sdrhip_agc_set_enabled(_plan, 0, enabled ? 1 : 0), "AGC");
  }
  /** The current gain factor: the node's own on the device once it is configured. */
  inline float gain() const {
    float g = _gain;
    if (_plan) detail::configCheck(sdrhip_agc_get_state(_plan, &g, 0, 0, 1), "AGC");
    return g;
  }
  inline void setGain(float gain) {
    _gain = gain;
    if (_plan) detail::configCheck(sdrhip_agc_set_gain(_plan, 0, gain), "AGC");
  }
  inline double tau() const { return _tau; }
  /** The decay only; the running average and the gain go on (the reference's setTau). */
  inline void setTau(double tau) {
    _tau = float(tau);
    if (_plan) detail::configCheck(sdrhip_agc_set_lambda(_plan, 0, detail::agcLambda(_tau, _sampleRate, "AGC")), "AGC");
  }
  /** The running average of |x|: for AM or USB audio the channel's signal level. */
  inline float level() const {
    float s = _target;
    if (_plan) detail::configCheck(sdrhip_agc_get_state(_plan, 0, &s, 0, 1), "AGC");
    return s;
  }

  /** As the reference's: the average starts over at the target, the gain and the enabled flag stay. */
  virtual void config(const Config &src_cfg) {
    if (!src_cfg.hasType() || !src_cfg.hasSampleRate() || !src_cfg.hasBufferSize()) return;
    detail::checkType<Scalar>(src_cfg, "AGC node");
    const float g = gain();
    _sampleRate = src_cfg.sampleRate();
    detail::configCheck(sdrhip_agc_create(Device::get(_device), detail::AgcType<Scalar>::dtype, detail::agcLambda(_tau, _sampleRate, "AGC"),
                                          _target, 1, src_cfg.bufferSize(), _plan.out()), "AGC");
    setGain(g);
    enable(_enabled);
    _buffer.unref();
    _buffer = Buffer<Scalar>(src_cfg.bufferSize());
    this->setConfig(Config(Config::typeId<Scalar>(), src_cfg.sampleRate(), src_cfg.bufferSize(), 1));
  }

  virtual void process(const Buffer<Scalar> &buffer, bool allow_overwrite) {
    (void)allow_overwrite;
    if (!_plan) return;
    if (!detail::processOk(sdrhip_agc_process(_plan, buffer.data(), buffer.size(), 0, _buffer.data(), 0), "gpu::AGC")) return;
    this->send(_buffer.head(buffer.size()), false);
  }

protected:
  bool _enabled;
  float _tau, _target, _gain;
  double _sampleRate;
  int _device;
  detail::Handle<sdrhip_agc, sdrhip_agc_destroy> _plan;
  Buffer<Scalar> _buffer;
};

/** N AGC<Scalar> nodes over rows, host or device. Not a graph node: process() takes `channels` rows of n samples at a row
 * stride (0: n) and writes as many; processDev() does the same on device rows of this bank's device — behind a tuner bank's
 * device rows there is no host copy in between — and synchronises nothing. */
template <class Scalar>
class AGCBank {
public:
  /** The same tau and target (0: the type's default) on every row at sample rate Fs; maxIn: the longest call. */
  AGCBank(size_t channels, double Fs, double tau = 0.1, double target = 0, size_t maxIn = 65536, int device = 0)
    : _ctx(Device::get(device)), _C(channels), _Fs(Fs) {
    detail::configCheck(sdrhip_agc_create(_ctx, detail::AgcType<Scalar>::dtype, detail::agcLambda(tau, Fs, "AGCBank"),
                                          detail::agcTarget(detail::AgcType<Scalar>::dtype, target, "AGCBank"), int(channels), maxIn, _h.out()),
                        "AGCBank");
  }
  /** A time constant, a target (0: default) and an enabled flag per row. */
  AGCBank(double Fs, const std::vector<double> &tau, const std::vector<double> &target, const std::vector<bool> &enabled,
          size_t maxIn = 65536, int device = 0)
    : _ctx(Device::get(device)), _C(tau.size()), _Fs(Fs) {
    std::vector<float> l(_C ? _C : 1), t(_C ? _C : 1);
    std::vector<int> e(_C ? _C : 1, 1);
    for (size_t c = 0; c < _C; c++) {
      l[c] = detail::agcLambda(tau[c], Fs, "AGCBank");
      t[c] = detail::agcTarget(detail::AgcType<Scalar>::dtype, c < target.size() ? target[c] : 0, "AGCBank");
      e[c] = c < enabled.size() ? (enabled[c] ? 1 : 0) : 1;
    }
    detail::configCheck(sdrhip_agcbank_create(_ctx, detail::AgcType<Scalar>::dtype, l.data(), t.data(), e.data(), int(_C), maxIn, _h.out()),
                        "AGCBank");
  }
  virtual ~AGCBank() {
    sdrhip_ctx_synchronize(_ctx);
    _h.reset();
  }

  size_t channels() const { return _C; }
  sdrhip_ctx *context() const { return _ctx; }

  bool process(const Scalar *in, size_t n, size_t inStride, Scalar *out, size_t outStride) {
    return detail::processOk(sdrhip_agc_process(_h, in, n, inStride, out, outStride), "gpu::AGCBank");
  }
  bool processDev(const Scalar *inDev, size_t n, size_t inStride, Scalar *outDev, size_t outStride) {
    return detail::processOk(sdrhip_agc_process_dev(_h, inDev, n, inStride, outDev, outStride), "gpu::AGCBank");
  }

  /** A fresh node behind row c. */
  void setChannel(size_t c, double tau, double target = 0) {
    detail::configCheck(sdrhip_agc_set_channel(_h, int(c), detail::agcLambda(tau, _Fs, "AGCBank"),
                                               detail::agcTarget(detail::AgcType<Scalar>::dtype, target, "AGCBank")), "AGCBank");
  }
  void setTau(size_t c, double tau) { detail::configCheck(sdrhip_agc_set_lambda(_h, int(c), detail::agcLambda(tau, _Fs, "AGCBank")), "AGCBank"); }
  void enable(size_t c, bool on) { detail::configCheck(sdrhip_agc_set_enabled(_h, int(c), on ? 1 : 0), "AGCBank"); }
  void setGain(size_t c, float gain) { detail::configCheck(sdrhip_agc_set_gain(_h, int(c), gain), "AGCBank"); }
  /** gain and level (the running average of |x|) of every row behind the calls made so far. */
  void state(std::vector<float> &gain, std::vector<float> &level) {
    gain.resize(_C); level.resize(_C);
    detail::configCheck(sdrhip_agc_get_state(_h, gain.data(), level.data(), 0, int(_C)), "AGCBank");
  }
  void reset() { detail::configCheck(sdrhip_agc_reset(_h), "AGCBank"); }

protected:
  sdrhip_ctx *_ctx;
  size_t _C;
  double _Fs;
  detail::Handle<sdrhip_agc, sdrhip_agc_destroy> _h;
};

}  // namespace gpu
}  // namespace sdr
#endif
