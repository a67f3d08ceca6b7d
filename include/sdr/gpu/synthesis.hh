/* sdr/gpu/synthesis.hh — gpu::Synthesis: the polyphase synthesis bank (sdrhip_synthesis_*, include/sdrhip_synthesis.h has the
 * contract), the mirror of gpu::Channelizer: complex float channel rows, one per selected channel, onto ONE wideband stream at D
 * times the rows' rate. A Source of std::complex<float>. Its input is rows, not one stream, so it is no Sink: config(rate,
 * columns) makes the plan and process(rows, n, stride) takes the host rows of one round — one H2D copy per row block, two
 * launches, one D2H copy — and sends the n D samples as a view of the node's buffer; a round is dropped while a consumer still
 * holds the last one. processDev() runs the same plan on device rows of the node's device and synchronises nothing: the rows
 * gpu::Channelizer::processDev and the AGC, resampler and BPSK31 banks leave go in as they are.
 *
 * The rules of sdrhip_synthesis_create that need no device are checked by the constructor and throw ConfigError (the grid's
 * rules are channelizer.hh's checkGrid and checkSelection).
 */
#ifndef SDR_GPU_SYNTHESIS_HH
#define SDR_GPU_SYNTHESIS_HH

#include "channelizer.hh"
#include "../../sdrhip_synthesis.h"

namespace sdr {
namespace gpu {

namespace detail {
/** The synthesis bank's grid: M channels of an M-point transform, as the complex channelizer's. */
struct SynthesisGrid {
  static const char *name() { return "Synthesis"; }
  static const char *ruleM() { return " (2 ... 4096, prime factors up to 13)"; }
  static bool admitsM(size_t M) { return M >= 2 && M <= 4096; }
  static size_t transform(size_t M) { return M; }
  static size_t channels(size_t M) { return M; }
};
}  // namespace detail

class Synthesis : public Source {
public:
  /** M channels interpolated by D with the prototype low-pass `taps`; channels: the channel each input row belongs to, any
   * order, no duplicates (empty: all M in order). Checked here, ConfigError: 2 <= M <= 4096 with prime factors up to 13,
   * 1 <= D <= M, 1 <= taps.size() <= 64 D, every tap finite as a float, every channel in [0, M), once. */
  Synthesis(size_t M, size_t D, const std::vector<double> &taps, const std::vector<int> &channels = std::vector<int>(), int device = 0)
    : Source(), _M(M), _D(D), _taps(taps), _sel(channels), _device(device), _ctx(0), _cols(0) {
    detail::checkGrid<detail::SynthesisGrid>(M, D, taps, D < 1 || taps.size() <= 64 * D, "; at most 64 D taps");
    detail::checkSelection<detail::SynthesisGrid>(_sel, M);
  }
  virtual ~Synthesis() { _release(); }

  /** The rows taken, and the channel row i belongs to. */
  size_t rows() const { return _sel.size(); }
  int channel(size_t i) const { return _sel[i]; }
  sdrhip_ctx *context() const { return _ctx; }

  /** The plan for rounds of up to maxColumns columns of rows at rowRate; the output's Config is cf32 at rowRate D in buffers
   * of maxColumns D. ConfigError where the library refuses (the size rules that involve maxColumns, no device). */
  void config(double rowRate, size_t maxColumns) {
    _release();
    _ctx = Device::get(_device);
    detail::configCheck(sdrhip_synthesis_create(_ctx, int(_M), int(_D), _taps.data(), int(_taps.size()), maxColumns, _plan.out()), "Synthesis");
    detail::configCheck(sdrhip_synthesis_set_channels(_plan, _sel.data(), int(_sel.size())), "Synthesis");
    _cols = maxColumns;
    _din.alloc(_ctx, _sel.size() * _cols * sizeof(cf32), "Synthesis");
    _dout.alloc(_ctx, _cols * _D * sizeof(cf32), "Synthesis");
    _buffer = Buffer<cf32>(_cols * _D);
    this->setConfig(Config(Config::typeId<cf32>(), rowRate * double(_D), _cols * _D, 1));
  }

  /** One round: rows() host rows of n columns, row i at rows + i inStride (0: n). Sends the n D output samples; false where the
   * round was dropped (no plan, more than the configured columns, the last round's buffer still in use, a device error). */
  bool process(const cf32 *rows, size_t n, size_t inStride = 0) {
    if (!_plan || n > _cols) return false;
    if (n == 0) return true;
    if (!_buffer.isUnused()) {
      LogMessage msg(LOG_WARNING);
      msg << "gpu::Synthesis: output of the last round still in use downstream; round dropped";
      Logger::get().log(msg);
      return false;
    }
    if (inStride == 0) inStride = n;
    size_t got = 0;
    for (size_t i = 0; i < _sel.size(); i++)
      if (!detail::processOk(sdrhip_memcpy_h2d_async(_ctx, _din.as<cf32>() + i * n, rows + i * inStride, n * sizeof(cf32)), "gpu::Synthesis"))
        return false;
    if (!detail::processOk(sdrhip_synthesis_process_dev(_plan, _din.get(), n, n, _dout.get(), &got), "gpu::Synthesis") ||
        !detail::processOk(sdrhip_memcpy_d2h_async(_ctx, _buffer.data(), _dout.get(), got * sizeof(cf32)), "gpu::Synthesis") ||
        !detail::processOk(sdrhip_ctx_synchronize(_ctx), "gpu::Synthesis"))
      return false;
    this->send(_buffer.head(got), false);
    return true;
  }

  /** rows() device rows of n columns in (inStride in complex elements, 0: n), n D device samples out; two launches on the
   * context's stream, nothing is synchronised. After config() only. */
  bool processDev(const void *inDev, size_t n, size_t inStride, void *outDev, size_t *nOut) {
    return detail::processOk(sdrhip_synthesis_process_dev(_plan, inDev, n, inStride, outDev, nOut), "gpu::Synthesis");
  }

  /** A new prototype of the same length; the stream goes on. */
  void setTaps(const std::vector<double> &taps) {
    if (taps.size() != _taps.size()) {
      ConfigError err;
      err << "Synthesis: " << taps.size() << " taps where the node has " << _taps.size();
      throw err;
    }
    if (_plan) detail::configCheck(sdrhip_synthesis_set_taps(_plan, taps.data()), "Synthesis");
    _taps = taps;
  }
  /** As freshly configured, with the current parameters. */
  void reset() { if (_plan) detail::configCheck(sdrhip_synthesis_reset(_plan), "Synthesis"); }
  /** The columns taken since config() or reset(). */
  uint64_t consumed() const {
    uint64_t c = 0;
    if (_plan) detail::configCheck(sdrhip_synthesis_get_state(_plan, &c, 0, 0), "Synthesis");
    return c;
  }

protected:
  /** In this order: the device is idle before anything it may still use goes. */
  void _release() {
    if (_ctx) sdrhip_ctx_synchronize(_ctx);
    _plan.reset();
    _din.reset();
    _dout.reset();
    _buffer.unref();
  }

  size_t _M, _D;
  std::vector<double> _taps;
  std::vector<int> _sel;
  int _device;
  sdrhip_ctx *_ctx;
  detail::Handle<sdrhip_synthesis, sdrhip_synthesis_destroy> _plan;
  detail::DeviceMem _din, _dout;
  size_t _cols;
  Buffer<cf32> _buffer;
};

}  // namespace gpu
}  // namespace sdr
#endif
