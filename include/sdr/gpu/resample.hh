/* sdr/gpu/resample.hh — gpu::InpolSubSampler<iScalar, oScalar>, the drop-in for the reference's InpolSubSampler
 * (src/subsample.hh:194-288), and gpu::InpolSubSamplerBank<iScalar, oScalar>, N such nodes over rows in one launch, each row with
 * a ratio of its own (sdrhip_resample_*, include/sdrhip_resample.h has the contract).
 *
 * The type pairs are those that compile in the reference: float -> float, complex<float> -> complex<float>, int16_t -> int16_t
 * (the wrapping int16 accumulator) and complex<int16_t> -> complex<float>.
 *
 * Deviations from the reference: frac must lie in [0.125, 4096]; the output buffer holds the capacity of the source's buffer size
 * (the reference sizes it with the sample rate as a factor); and the interpolation table is the library's own design unless the
 * caller passes one (the reference's table, with its missing row, is data the tests keep).
 */
#ifndef SDR_GPU_RESAMPLE_HH
#define SDR_GPU_RESAMPLE_HH

#include "nodes.hh"
#include "psk31.hh"
#include "../../sdrhip_resample.h"

#include <vector>

namespace sdr {
namespace gpu {

namespace detail {
template <class I, class O> struct ResampleType;
template <> struct ResampleType<float, float> { enum { dtype = SDRHIP_RESAMPLE_F32, components = 1 }; };
template <> struct ResampleType<std::complex<float>, std::complex<float> > { enum { dtype = SDRHIP_RESAMPLE_CF32, components = 2 }; };
template <> struct ResampleType<int16_t, int16_t> { enum { dtype = SDRHIP_RESAMPLE_I16, components = 1 }; };
template <> struct ResampleType<std::complex<int16_t>, std::complex<float> > { enum { dtype = SDRHIP_RESAMPLE_CS16_CF32, components = 2 }; };
}  // namespace detail

/** InpolSubSampler<iScalar, oScalar>(frac) with the reference's surface: a Sink of iScalar, a Source of oScalar at
 * sampleRate / frac. table: 129 x 8 interpolation taps (0: the library's design). */
template <class iScalar, class oScalar = iScalar>
class InpolSubSampler : public Sink<iScalar>, public Source {
public:
  InpolSubSampler(float frac, const float *table = 0, int device = 0)
    : Sink<iScalar>(), Source(), _frac(frac), _table(detail::inpolTaps(table, "InpolSubSampler")), _device(device) {
    if (!(_frac >= 0.125f && _frac <= 4096.f)) {
      ConfigError err;
      err << "Can not configure InpolSubSample node: Sample rate fraction must lie in [0.125, 4096]!"
          << " Fraction given: " << _frac;
      throw err;
    }
  }
  virtual ~InpolSubSampler() { _buffer.unref(); }

  virtual void config(const Config &src_cfg) {
    if (!src_cfg.hasType() || !src_cfg.hasBufferSize()) return;
    detail::checkType<iScalar>(src_cfg, "InpolSubSample node", "buffer type");
    detail::configCheck(sdrhip_resample_create(Device::get(_device), detail::ResampleType<iScalar, oScalar>::dtype, _frac, _table.data(), 1,
                                               src_cfg.bufferSize(), _plan.out()), "InpolSubSampler");
    size_t cap = 0;
    detail::configCheck(sdrhip_resample_out_capacity(_plan, src_cfg.bufferSize(), &cap), "InpolSubSampler");
    _buffer.unref();
    _buffer = Buffer<oScalar>(cap ? cap : 1);
    this->setConfig(Config(Config::typeId<oScalar>(), src_cfg.sampleRate() / _frac, cap ? cap : 1, 1));
  }

  virtual void process(const Buffer<iScalar> &buffer, bool allow_overwrite) {
    (void)allow_overwrite;
    if (!_plan) return;
    uint32_t count = 0;
    if (!detail::processOk(sdrhip_resample_process(_plan, buffer.data(), buffer.size(), 0, _buffer.data(), _buffer.size(), &count),
                           "gpu::InpolSubSampler"))
      return;
    if (count > 0) this->send(_buffer.head(count), false);
  }

  /** mu of the node behind the buffers processed so far (0 before config()). */
  float mu() const {
    float m = 0;
    if (_plan) detail::configCheck(sdrhip_resample_get_state(_plan, 0, &m, 0, 0, 1), "InpolSubSampler");
    return m;
  }

protected:
  float _frac;
  std::vector<float> _table;
  int _device;
  detail::Handle<sdrhip_resample, sdrhip_resample_destroy> _plan;
  Buffer<oScalar> _buffer;
};

/** N InpolSubSampler<iScalar, oScalar> nodes over rows, host or device. Not a graph node: process() takes `channels` rows of n
 * samples at a row stride (0: n) and writes each row's outputs (row stride outStride output elements, 0: outCapacity(n)) and
 * counts; processDev() does the same on device rows of this bank's device — a tuner bank's rows as it left them, no host copy
 * in between — and synchronises nothing. */
template <class iScalar, class oScalar = iScalar>
class InpolSubSamplerBank {
public:
  /** The same frac on every row; maxIn: the longest call; table: 129 x 8 taps (0: the library's design). */
  InpolSubSamplerBank(size_t channels, float frac, size_t maxIn = 65536, const float *table = 0, int device = 0)
    : _ctx(Device::get(device)), _C(channels) {
    const std::vector<float> t = detail::inpolTaps(table, "InpolSubSamplerBank");
    detail::configCheck(sdrhip_resample_create(_ctx, detail::ResampleType<iScalar, oScalar>::dtype, frac, t.data(), int(channels), maxIn, _h.out()),
                        "InpolSubSamplerBank");
  }
  /** A frac per row. */
  InpolSubSamplerBank(const std::vector<float> &frac, size_t maxIn = 65536, const float *table = 0, int device = 0)
    : _ctx(Device::get(device)), _C(frac.size()) {
    const std::vector<float> t = detail::inpolTaps(table, "InpolSubSamplerBank");
    detail::configCheck(sdrhip_resamplebank_create(_ctx, detail::ResampleType<iScalar, oScalar>::dtype, frac.data(), t.data(), int(_C), maxIn,
                                                   _h.out()), "InpolSubSamplerBank");
  }
  virtual ~InpolSubSamplerBank() {
    sdrhip_ctx_synchronize(_ctx);
    _h.reset();
  }

  size_t channels() const { return _C; }
  sdrhip_ctx *context() const { return _ctx; }
  /** The most outputs a row writes in a call of n samples: the smallest output-row stride. */
  size_t outCapacity(size_t n) const {
    size_t cap = 0;
    detail::configCheck(sdrhip_resample_out_capacity(_h, n, &cap), "InpolSubSamplerBank");
    return cap;
  }

  bool process(const iScalar *in, size_t n, size_t inStride, oScalar *out, size_t outStride, uint32_t *counts) {
    return detail::processOk(sdrhip_resample_process(_h, in, n, inStride, out, outStride, counts), "gpu::InpolSubSamplerBank");
  }
  bool processDev(const void *inDev, size_t n, size_t inStride, void *outDev, size_t outStride, uint32_t *countsDev) {
    return detail::processOk(sdrhip_resample_process_dev(_h, inDev, n, inStride, outDev, outStride, countsDev), "gpu::InpolSubSamplerBank");
  }

  /** A fresh node with this frac behind row c. */
  void setChannel(size_t c, float frac) { detail::configCheck(sdrhip_resample_set_channel(_h, int(c), frac), "InpolSubSamplerBank"); }
  void reset() { detail::configCheck(sdrhip_resample_reset(_h), "InpolSubSamplerBank"); }
  /** mu of every row and its line (8 x components values per row, oldest first, in the output's scalar type) behind the calls
   * made so far. */
  void state(std::vector<float> &mu, std::vector<oScalar> &line) {
    mu.resize(_C); line.resize(_C * 8);
    const bool i16 = int(detail::ResampleType<iScalar, oScalar>::dtype) == SDRHIP_RESAMPLE_I16;
    detail::configCheck(sdrhip_resample_get_state(_h, 0, mu.data(), i16 ? 0 : reinterpret_cast<float *>(line.data()),
                                                  i16 ? reinterpret_cast<int16_t *>(line.data()) : 0, int(_C)), "InpolSubSamplerBank");
  }

protected:
  sdrhip_ctx *_ctx;
  size_t _C;
  detail::Handle<sdrhip_resample, sdrhip_resample_destroy> _h;
};

}  // namespace gpu
}  // namespace sdr
#endif
