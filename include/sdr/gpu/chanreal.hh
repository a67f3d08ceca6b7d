/* sdr/gpu/chanreal.hh — the channelizer family for a REAL-sampled antenna stream (include/sdrhip_chanreal.h has the contract) as
 * graph nodes, each a Sink of Scalar — int16_t or float: a direct-sampling front end, an IF tap or a sound card:
 *   gpu::RealChannelizer<Scalar>        one Source per selected channel, Buffer<std::complex<float>> at sampleRate / D
 *   gpu::RealAudioChannelizer<Scalar>   one Source per selected channel, Buffer<int16_t> audio (FM, AM or USB per row)
 *   gpu::RealChannelPower<Scalar>       no rows: sums of |y_k|^2, levels, flags and occupied()
 * The channels are 0 ... M / 2 (channel M - k is the conjugate of channel k), so selections, modes, gains, thresholds, sums, levels
 * and flags have M / 2 + 1 entries. They are gpu::ChannelizerNode, gpu::AudioChannelizerNode and gpu::ChannelPowerNode
 * (channelizer.hh, chanaudio.hh, chanpower.hh) on the real grid: config(), process(), processDev() and the setters and getters
 * are those classes', so per buffer there is one H2D copy of the real row, the complex nodes' launches and one D2H copy, and
 * processDev() runs the same plan on device rows and synchronises nothing.
 */
#ifndef SDR_GPU_CHANREAL_HH
#define SDR_GPU_CHANREAL_HH

#include "channelizer.hh"
#include "chanaudio.hh"
#include "chanpower.hh"
#include "../../sdrhip_chanreal.h"

namespace sdr {
namespace gpu {

namespace detail {
template <class Scalar> struct RealChannelizerType;
template <> struct RealChannelizerType<int16_t> { enum { dtype = SDRHIP_CHANREAL_S16 }; };
template <> struct RealChannelizerType<float> { enum { dtype = SDRHIP_CHANREAL_F32 }; };

/** The real-input grid: M even, M / 2 + 1 channels of an M / 2-point transform, sdrhip_chanreal_channelizer_create. */
template <class Scalar> struct RealGrid {
  typedef Scalar In;
  typedef ChannelizerApi Api;
  static const char *name() { return "RealChannelizer"; }
  static const char *ruleM() { return " (even, 4 ... 4096, M / 2 with prime factors up to 13)"; }
  static bool admitsM(size_t M) { return M >= 4 && M <= 4096 && M % 2 == 0; }
  static size_t transform(size_t M) { return M / 2; }
  static size_t channels(size_t M) { return M / 2 + 1; }
  static int create(sdrhip_ctx *ctx, int M, int D, const double *taps, int nTaps, size_t maxIn, sdrhip_channelizer **out) {
    return sdrhip_chanreal_channelizer_create(ctx, RealChannelizerType<Scalar>::dtype, M, D, taps, nTaps, maxIn, out);
  }
};
template <class Scalar> struct RealAudioGrid : RealGrid<Scalar> {
  typedef ChanAudioApi Api;
  static const char *name() { return "RealAudioChannelizer"; }
  static int create(sdrhip_ctx *ctx, int M, int D, const double *taps, int nTaps, size_t maxIn, const int *modes, const float *gains,
                    sdrhip_chanaudio **out) {
    return sdrhip_chanreal_audio_create(ctx, RealChannelizerType<Scalar>::dtype, M, D, taps, nTaps, maxIn, modes, gains, out);
  }
};
template <class Scalar> struct RealPowerGrid : RealGrid<Scalar> {
  typedef ChanPowerApi Api;
  static const char *name() { return "RealChannelPower"; }
  static int create(sdrhip_ctx *ctx, int M, int D, const double *taps, int nTaps, size_t maxIn, double alpha, sdrhip_chanpower **out) {
    return sdrhip_chanreal_power_create(ctx, RealChannelizerType<Scalar>::dtype, M, D, taps, nTaps, maxIn, alpha, out);
  }
};
}  // namespace detail

template <class Scalar>
class RealChannelizer : public ChannelizerNode< detail::RealGrid<Scalar> > {
public:
  /** M / 2 + 1 channels decimated by D with the prototype low-pass `taps`; channels: the channels to deliver, any order, no
   * duplicates (empty: 0 ... M / 2 in order). The rules of sdrhip_chanreal_channelizer_create are checked here and throw
   * ConfigError: M even, 4 <= M <= 4096, M / 2 with prime factors up to 13, 1 <= D <= M, 1 <= taps.size() <= 64 M, every tap
   * finite as a float, every channel in [0, M / 2], once. */
  RealChannelizer(size_t M, size_t D, const std::vector<double> &taps, const std::vector<int> &channels = std::vector<int>(), int device = 0)
    : ChannelizerNode< detail::RealGrid<Scalar> >(M, D, taps, channels, device) {}
};

template <class Scalar>
class RealAudioChannelizer : public AudioChannelizerNode< detail::RealAudioGrid<Scalar> > {
public:
  /** As RealChannelizer, with modes[i], gains[i]: row i's demodulator (SDRHIP_EPI_FM, _AM or _USB) and gain (empty: FM, 1); the
   * rules of sdrhip_chanreal_audio_create are checked here and throw ConfigError: those of RealChannelizer, a mode and a gain per
   * row, every mode one of the three, every gain finite. */
  RealAudioChannelizer(size_t M, size_t D, const std::vector<double> &taps, const std::vector<int> &channels = std::vector<int>(),
                       const std::vector<int> &modes = std::vector<int>(), const std::vector<float> &gains = std::vector<float>(), int device = 0)
    : AudioChannelizerNode< detail::RealAudioGrid<Scalar> >(M, D, taps, channels, modes, gains, device) {}
};

template <class Scalar>
class RealChannelPower : public ChannelPowerNode< detail::RealPowerGrid<Scalar> > {
public:
  /** M / 2 + 1 channels (channels()) decimated by D, the level following the buffers' means with the factor alpha; the rules of
   * sdrhip_chanreal_power_create are checked here and throw ConfigError: those of RealChannelizer for M, D and taps, 0 < alpha <= 1. */
  RealChannelPower(size_t M, size_t D, const std::vector<double> &taps, double alpha = 0.25, int device = 0)
    : ChannelPowerNode< detail::RealPowerGrid<Scalar> >(M, D, taps, alpha, device) {}
};

}  // namespace gpu
}  // namespace sdr
#endif
