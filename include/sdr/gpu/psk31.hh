/* sdr/gpu/psk31.hh — gpu::BPSK31<Scalar>, the drop-in for the reference's BPSK31<int16_t> / BPSK31<float> (src/psk31.hh:16-291);
 * gpu::BPSK31Bank<Scalar>, N such demodulators over rows in one launch (sdrhip_psk31_*, include/sdrhip_psk31.h); and sdr::Varicode,
 * the host-only decoder of the bit stream (src/psk31.hh:299-318).
 *
 * Deviations from the reference (sdrhip_psk31.h has the contract): the carrier's sine and cosine are a defined sequence of double
 * operations, not the C library's sincosf; a buffer longer than one second is served like any other; and the interpolation table
 * is the library's own design unless the caller passes one (the reference's table, with its missing row, is data the tests keep).
 */
#ifndef SDR_GPU_PSK31_HH
#define SDR_GPU_PSK31_HH

#include "nodes.hh"
#include "../../sdrhip_psk31.h"

#include <map>
#include <string>
#include <vector>

namespace sdr {
namespace gpu {

namespace detail {
template <class Scalar> struct PskType;
template <> struct PskType<int16_t> { enum { dtype = SDRHIP_PSK31_CS16 }; };
template <> struct PskType<float> { enum { dtype = SDRHIP_PSK31_CF32 }; };
inline std::vector<float> inpolTaps(const float *table, const char *what) {
  std::vector<float> t(129 * 8);
  if (table) t.assign(table, table + 129 * 8);
  else configCheck(sdrhip_design_inpol_taps(t.data()), what);
  return t;
}
}  // namespace detail

/** BPSK31<Scalar>(dF) with the reference's surface: a Sink of complex<Scalar> at 2000 Hz or more, a Source of uint8_t bits at
 * 31.25 Hz. table: 129 x 8 interpolation taps (0: the library's design). */
template <class Scalar>
class BPSK31 : public Sink< std::complex<Scalar> >, public Source {
public:
  BPSK31(double dF = 0.1, const float *table = 0, int device = 0)
    : _dF(dF), _table(detail::inpolTaps(table, "BPSK31")), _device(device) {}
  virtual ~BPSK31() { _buffer.unref(); }

  virtual void config(const Config &src_cfg) {
    if (!src_cfg.hasType() || !src_cfg.hasSampleRate() || !src_cfg.hasBufferSize()) return;
    detail::checkType< std::complex<Scalar> >(src_cfg, "BPSK31");
    const double Fs = src_cfg.sampleRate();
    if (2000 > Fs) {
      ConfigError err;
      err << "Can not configure BPSK31: Input sample rate too low! The BPSK31 node requires at "
          << "least a sample rate of 2000Hz, got " << Fs << "Hz";
      throw err;
    }
    detail::configCheck(sdrhip_psk31_create(Device::get(_device), detail::PskType<Scalar>::dtype, Fs, _dF, _table.data(), 1,
                                            src_cfg.bufferSize(), _plan.out()), "BPSK31");
    size_t cap = 0;
    detail::configCheck(sdrhip_psk31_out_capacity(_plan, src_cfg.bufferSize(), &cap), "BPSK31");
    _buffer.unref();
    _buffer = Buffer<uint8_t>(cap ? cap : 1);
    this->setConfig(Config(Config::typeId<uint8_t>(), 31.25, src_cfg.bufferSize(), 1));
  }

  virtual void process(const Buffer< std::complex<Scalar> > &buffer, bool allow_overwrite) {
    (void)allow_overwrite;
    if (!_plan) return;
    uint32_t count = 0;
    if (!detail::processOk(sdrhip_psk31_process(_plan, buffer.data(), buffer.size(), 0, reinterpret_cast<uint8_t *>(_buffer.data()),
                                                     _buffer.size(), &count), "gpu::BPSK31"))
      return;
    if (count > 0) this->send(_buffer.head(count), false);
  }

  /** P, F, mu, omega of the node behind the buffers processed so far (zeros before config()). */
  void state(float &P, float &F, float &mu, float &omega) const {
    P = F = mu = omega = 0;
    if (_plan) detail::configCheck(sdrhip_psk31_get_state(_plan, &P, &F, &mu, &omega, 0, 0, 1), "BPSK31");
  }

protected:
  double _dF;
  std::vector<float> _table;
  int _device;
  detail::Handle<sdrhip_psk31, sdrhip_psk31_destroy> _plan;
  Buffer<uint8_t> _buffer;
};

/** N BPSK31<Scalar> demodulators over rows, host or device. Not a graph node: process() takes `channels` rows of n complex samples
 * at a row stride (0: n) and writes each row's bits (one byte per bit, row stride outStride bytes, 0: capacity(n)) and counts;
 * processDev() does the same on device rows of this bank's device — a tuner bank's SDRHIP_EPI_NONE rows as it left them, no host
 * copy in between — and synchronises nothing. */
template <class Scalar>
class BPSK31Bank {
public:
  /** The same dF on every row at sample rate Fs; maxIn: the longest call; table: 129 x 8 taps (0: the library's design). */
  BPSK31Bank(size_t channels, double Fs, double dF = 0.1, size_t maxIn = 65536, const float *table = 0, int device = 0)
    : _ctx(Device::get(device)), _C(channels) {
    const std::vector<float> t = detail::inpolTaps(table, "BPSK31Bank");
    detail::configCheck(sdrhip_psk31_create(_ctx, detail::PskType<Scalar>::dtype, Fs, dF, t.data(), int(channels), maxIn, _h.out()), "BPSK31Bank");
  }
  /** A dF per row. */
  BPSK31Bank(double Fs, const std::vector<float> &dF, size_t maxIn = 65536, const float *table = 0, int device = 0)
    : _ctx(Device::get(device)), _C(dF.size()) {
    const std::vector<float> t = detail::inpolTaps(table, "BPSK31Bank");
    detail::configCheck(sdrhip_psk31bank_create(_ctx, detail::PskType<Scalar>::dtype, Fs, dF.data(), t.data(), int(_C), maxIn, _h.out()),
                        "BPSK31Bank");
  }
  virtual ~BPSK31Bank() {
    sdrhip_ctx_synchronize(_ctx);
    _h.reset();
  }

  size_t channels() const { return _C; }
  sdrhip_ctx *context() const { return _ctx; }
  /** The most bits a row writes in a call of n samples: the smallest bit-row stride. */
  size_t capacity(size_t n) const {
    size_t cap = 0;
    detail::configCheck(sdrhip_psk31_out_capacity(_h, n, &cap), "BPSK31Bank");
    return cap;
  }

  bool process(const std::complex<Scalar> *in, size_t n, size_t inStride, uint8_t *bits, size_t outStride, uint32_t *counts) {
    return detail::processOk(sdrhip_psk31_process(_h, in, n, inStride, bits, outStride, counts), "gpu::BPSK31Bank");
  }
  bool processDev(const void *inDev, size_t n, size_t inStride, uint8_t *bitsDev, size_t outStride, uint32_t *countsDev) {
    return detail::processOk(sdrhip_psk31_process_dev(_h, inDev, n, inStride, bitsDev, outStride, countsDev), "gpu::BPSK31Bank");
  }

  /** A fresh node with range dF behind row c. */
  void setChannel(size_t c, double dF) { detail::configCheck(sdrhip_psk31_set_channel(_h, int(c), dF), "BPSK31Bank"); }
  void reset() { detail::configCheck(sdrhip_psk31_reset(_h), "BPSK31Bank"); }
  /** P, F, mu, omega of every row behind the calls made so far. */
  void state(std::vector<float> &P, std::vector<float> &F, std::vector<float> &mu, std::vector<float> &omega) {
    P.resize(_C); F.resize(_C); mu.resize(_C); omega.resize(_C);
    detail::configCheck(sdrhip_psk31_get_state(_h, P.data(), F.data(), mu.data(), omega.data(), 0, 0, int(_C)), "BPSK31Bank");
  }

protected:
  sdrhip_ctx *_ctx;
  size_t _C;
  detail::Handle<sdrhip_psk31, sdrhip_psk31_destroy> _h;
};

}  // namespace gpu

/** The Varicode decoder of PSK31 on the host: a Sink of uint8_t bits, a Source of the decoded characters (no sample rate).
 * The alphabet is the published PSK31 table (every code starts and ends with 1 and holds no 00; 00 separates codes), restricted
 * to what the reference decodes and with the values it decodes them by; EOT decodes as '\n', a code outside the table is dropped.
 * A code cut by the end of a buffer is finished by the next. */
class Varicode : public Sink<uint8_t>, public Source {
public:
  Varicode() : Sink<uint8_t>(), Source(), _value(0) {
    static const char *const codes[] = {
      "\n", "11101", "\n", "1011101011", "\r", "11111", " ", "1", "!", "1111111111", "\"", "101011111", "#", "1111110101", "$", "111011011",
      "%", "11011010101", "&", "1010111011", "'", "1101111111", ")", "111110111", "*", "101101111", "+", "1111011111", "-", "1110101",
      ".", "1010111", "/", "1110101111", "0", "10110111", "1", "10111101", "2", "11101101", "3", "111111111", "4", "101110111",
      "5", "1101011011", "6", "101101011", "7", "1110101101", "8", "110101011", "9", "1110110111", ":", "11110101", ";", "110111101",
      "<", "111101101", "=", "1010101", ">", "111010111", "?", "1010101111", "@", "1010111101", "A", "1111101", "B", "11101011",
      "C", "10101101", "D", "10110101", "E", "1110111", "F", "11011011", "G", "11111101", "H", "101010101", "I", "1111111",
      "J", "111111101", "K", "101111101", "L", "11010111", "M", "10111011", "N", "11011101", "O", "10101011", "P", "11010101",
      "Q", "111011101", "R", "10101111", "S", "1101111", "T", "1101101", "U", "101010111", "V", "110110101", "W", "101011101",
      "X", "101110101", "Y", "101111011", "Z", "1010101101", "[", "11111011", "\\", "111101111", "]", "111111011", "^", "1010111111",
      "_", "101101101", "`", "1011011111", "a", "1011", "b", "1011111", "c", "101111", "d", "101101", "e", "11", "f", "111101",
      "g", "1011011", "h", "101011", "i", "1101", "j", "111101011", "k", "10111111", "l", "11011", "m", "111011", "n", "1111", "o", "111",
      "p", "111111", "q", "110111111", "r", "10101", "s", "10111", "t", "101", "u", "110111", "v", "1111011", "w", "1101011",
      "x", "11011111", "y", "1011101", "z", "111010101", "{", "1010110111", "|", "110111011", "}", "1010110101", "~", "1011010111", 0};
    for (size_t i = 0; codes[i]; i += 2) {
      uint16_t v = 0;
      for (const char *p = codes[i + 1]; *p; p++) v = uint16_t((v << 1) | (*p == '1'));
      _table[v] = codes[i][0];
    }
  }
  virtual ~Varicode() { _buffer.unref(); }

  virtual void config(const Config &src_cfg) {
    if (!src_cfg.hasType() || !src_cfg.hasBufferSize()) return;
    gpu::detail::checkType<uint8_t>(src_cfg, "Varicode");
    _value = 0;
    // (a character needs at least three bits: 1 and the 00 behind it)
    _buffer.unref();
    _buffer = Buffer<uint8_t>(src_cfg.bufferSize() / 3 + 1);
    this->setConfig(Config(Config::typeId<uint8_t>(), 0, _buffer.size(), 1));
  }

  virtual void process(const Buffer<uint8_t> &buffer, bool allow_overwrite) {
    (void)allow_overwrite;
    size_t o = 0;
    for (size_t i = 0; i < buffer.size(); i++) {
      _value = uint16_t((_value << 1) | (buffer[i] & 1));
      if (0 == (_value & 3)) {
        const std::map<uint16_t, char>::const_iterator it = _table.find(uint16_t(_value >> 2));
        if (it != _table.end() && o < _buffer.size()) _buffer[o++] = uint8_t(it->second);
        _value = 0;
      }
    }
    if (o) this->send(_buffer.head(o), false);
  }

protected:
  uint16_t _value;
  Buffer<uint8_t> _buffer;
  std::map<uint16_t, char> _table;
};

}  // namespace sdr
#endif
