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
 * The node's body is gpu::AudioChannelizerNode<Grid>: detail::RowNode (channelizer.hh) with int16 rows, plus the rows' modes and
 * gains. Grid says what the complex node and the real-input one of chanreal.hh (gpu::RealAudioChannelizer<Scalar>) differ in.
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
/** What the node bodies call of sdrhip_chanaudio.h. */
struct ChanAudioApi {
  typedef sdrhip_chanaudio Plan;
  static int destroy(Plan *p) { return sdrhip_chanaudio_destroy(p); }
  static int setChannels(Plan *p, const int *idx, int n) { return sdrhip_chanaudio_set_channels(p, idx, n); }
  static int processDev(Plan *p, const void *in, size_t n, void *out, size_t stride, size_t *nOut) {
    return sdrhip_chanaudio_process_dev(p, in, n, out, stride, nOut);
  }
  static int setTaps(Plan *p, const double *taps) { return sdrhip_chanaudio_set_taps(p, taps); }
  static int reset(Plan *p) { return sdrhip_chanaudio_reset(p); }
  static int consumed(Plan *p, uint64_t *c) { return sdrhip_chanaudio_get_state(p, c, 0, 0, 0, 0); }
};

/** The complex audio node's grid: detail::ComplexGrid with sdrhip_chanaudio_create (modes and gains: one per channel). */
template <class Scalar> struct ComplexAudioGrid : ComplexGrid<Scalar> {
  typedef ChanAudioApi Api;
  static const char *name() { return "AudioChannelizer"; }
  static int create(sdrhip_ctx *ctx, int M, int D, const double *taps, int nTaps, size_t maxIn, const int *modes, const float *gains,
                    sdrhip_chanaudio **out) {
    return sdrhip_chanaudio_create(ctx, ChannelizerType<Scalar>::dtype, M, D, taps, nTaps, maxIn, modes, gains, out);
  }
};
}  // namespace detail

template <class Grid>
class AudioChannelizerNode : public detail::RowNode<Grid, int16_t> {
public:
  /** M, D, taps, channels, modes and gains as gpu::AudioChannelizer and gpu::RealAudioChannelizer say; the grid's rules are
   * checked here and throw ConfigError. */
  AudioChannelizerNode(size_t M, size_t D, const std::vector<double> &taps, const std::vector<int> &channels, const std::vector<int> &modes,
                       const std::vector<float> &gains, int device)
    : detail::RowNode<Grid, int16_t>(M, D, taps, channels, device), _modes(modes), _gains(gains) {
    const std::vector<int> &sel = this->_sel;
    if (_modes.empty()) _modes.assign(sel.size(), int(SDRHIP_EPI_FM));
    if (_gains.empty()) _gains.assign(sel.size(), 1.0f);
    bool ok = _modes.size() == sel.size() && _gains.size() == sel.size();
    for (size_t i = 0; ok && i < sel.size(); i++)
      ok = (_modes[i] == SDRHIP_EPI_FM || _modes[i] == SDRHIP_EPI_AM || _modes[i] == SDRHIP_EPI_USB) && std::isfinite(_gains[i]);
    if (!ok) {
      ConfigError err;
      err << "Can not configure " << Grid::name() << " node: " << _modes.size() << " modes and " << _gains.size() << " gains for " << sel.size()
          << " rows (one each; SDRHIP_EPI_FM, _AM or _USB; finite gains)";
      throw err;
    }
    this->_makeOuts();
  }

  int mode(size_t i) const { return _modes[i]; }
  float gain(size_t i) const { return _gains[i]; }
  /** Row i's demodulator from now on (the row starts from last = 0) / its gain; before config() they are only noted. */
  void setMode(size_t i, int mode) {
    if (this->_plan) detail::configCheck(sdrhip_chanaudio_set_mode(this->_plan, int(i), mode), Grid::name());
    _modes.at(i) = mode;
  }
  void setGain(size_t i, float gain) {
    if (this->_plan) detail::configCheck(sdrhip_chanaudio_set_gain(this->_plan, int(i), gain), Grid::name());
    _gains.at(i) = gain;
  }

protected:
  virtual int _create() {
    const std::vector<int> &sel = this->_sel;
    std::vector<int> modes(this->_K, int(SDRHIP_EPI_FM));   // per channel: the rows' own, FM and 1 elsewhere
    std::vector<float> gains(this->_K, 1.0f);
    for (size_t i = 0; i < sel.size(); i++) { modes[size_t(sel[i])] = _modes[i]; gains[size_t(sel[i])] = _gains[i]; }
    return Grid::create(this->_ctx, int(this->_M), int(this->_D), this->_taps.data(), int(this->_taps.size()), this->_bs, modes.data(),
                        gains.data(), this->_plan.out());
  }

  std::vector<int> _modes;
  std::vector<float> _gains;
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
