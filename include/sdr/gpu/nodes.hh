// nodes.hh — MI355X nodes behind libsdr's node API (header-only; link with -lsdrhip).
//
// Every class here is an ordinary sdr::Sink<T> + sdr::Source with the reference node's name,
// constructor arguments, config()/process() behaviour, ownership and error rules, so it can replace
// the CPU node in an existing graph:
//   sdr::gpu::IQBaseBand<int16_t>           <->  sdr::IQBaseBand<int16_t>            reference src/baseband.hh:22-293
//   sdr::gpu::FIRLowPass<complex<int16|float>>  <->  sdr::FIRLowPass<...>            src/firfilter.hh:117-289
//   sdr::gpu::FMDemod<int16_t>, AMDemod<S>, USBDemod<S>  <->  same names             src/demod.hh:18-264
//   sdr::gpu::SubSample<complex<...>>       <->  sdr::SubSample<...>                 src/subsample.hh:16-116
//   sdr::gpu::FSKDetector, ASKDetector<int16_t>, BitStream  <->  same names          src/fsk.hh:18-171
//   sdr::gpu::FilterSink<float|double>      <->  sdr::FilterSink<Scalar>             src/filternode.hh:32-99
//   sdr::gpu::FilterSource<float|double>    <->  sdr::FilterSource<Scalar>           src/filternode.hh:103-227
//   sdr::gpu::FilterNode<float|double>      <->  sdr::FilterNode<Scalar>             src/filternode.hh:230-284
//   sdr::gpu::FFT, FFTPlan<float|double>    <->  sdr::FFT, sdr::FFTPlan<...>        src/fftplan.hh, src/fftplan_fftw3.hh
//   sdr::gpu::ChannelBank<int16_t>          many IQBaseBand(+demod) channels in ONE batched kernel launch;
//                                           sink(c)/source(c) per channel like Combine::sink(i) (src/combine.hh:66-150)
// Rules reproduced: config() returns silently while the upstream Config is incomplete and throws
// ConfigError on a type mismatch; the output buffer is owned by the node, allocated in config(),
// reused only when isUnused(), otherwise the input is dropped; a node writes into its input only
// when allow_overwrite; views (out.head(n)) are sent, never copies; process() never throws (device
// errors are logged at LOG_ERROR and the buffer is dropped).
//
// What the nodes share is written once, in namespace detail at the head of the file: the type check of config()
// (checkType), the owners of device plans, device memory and pinned registrations (Handle, DeviceMem, Pinned: a node
// that has one cannot be copied), the designed tap / LUT vectors, the send rule of a fused demodulator
// (sendDemodulated), the device hand-off between two gpu nodes (HandoffScope, handoffFor) and, further down, the one
// state machine of the int16 baseband plans (Bb16: IQBaseBand<int16_t|uint8_t|int8_t> and BaseBand<int16_t>).
//
// The header compiles against this repository's core (include/sdr/node.hh) or, when the
// reference's own node.hh was included first, against the reference core unchanged.
#ifndef SDR_GPU_NODES_HH
#define SDR_GPU_NODES_HH

#if !defined(__SDR_NODE_HH__) && !defined(SDR_CORE_NODE_HH)
#include "../node.hh"
#include "../logger.hh"
#endif

#include <algorithm>
#include <complex>
#include <cstring>
#include <list>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../sdrhip.h"
#include "design.hh"

namespace sdr {
namespace gpu {

typedef std::complex<int16_t> cs16;
typedef std::complex<float> cf32;

/** One shared device context per HIP device. Throws ConfigError when there is no GPU (no CPU fallback). */
class Device {
public:
  static sdrhip_ctx *get(int device = 0) {
    static std::map<int, sdrhip_ctx *> ctxs;
    std::map<int, sdrhip_ctx *>::iterator it = ctxs.find(device);
    if (it != ctxs.end()) return it->second;
    sdrhip_ctx *c = 0;
    const int rc = sdrhip_ctx_create(device, 0, &c);
    if (rc != SDRHIP_OK) {
      ConfigError err;
      err << "sdr::gpu: can not open HIP device " << device << ": " << sdrhip_strerror(rc) << " (" << sdrhip_last_error() << ")";
      throw err;
    }
    ctxs[device] = c;
    return c;
  }
};

namespace detail {
inline void configCheck(int rc, const char *what) {
  if (rc == SDRHIP_OK) return;
  ConfigError err;
  err << "Can not configure " << what << ": " << sdrhip_strerror(rc) << " (" << sdrhip_last_error() << ")";
  throw err;
}
inline bool processOk(int rc, const char *what) {
  if (rc == SDRHIP_OK) return true;
  LogMessage msg(LOG_ERROR);
  msg << what << ": drop buffer: " << sdrhip_strerror(rc) << " (" << sdrhip_last_error() << ")";
  Logger::get().log(msg);
  return false;
}
/** The type check of every config(), after the node's own guard for an incomplete Config: ConfigError unless the upstream
 * type is `want`. The message names `shown` as the expected type (BitStream's differs from the one it compares with). */
inline void checkType(const Config &cfg, Config::Type want, Config::Type shown, const char *what, const char *noun = "type") {
  if (want == cfg.type()) return;
  ConfigError err;
  err << "Can not configure " << what << ": Invalid " << noun << " " << cfg.type() << ", expected " << shown;
  throw err;
}
template <class T> inline void checkType(const Config &cfg, const char *what, const char *noun = "type") {
  checkType(cfg, Config::typeId<T>(), Config::typeId<T>(), what, noun);
}

/** The library's names for a complex sample type. */
template <class T> struct TypeTag;
template <> struct TypeTag<cs16> { enum { dtype = SDRHIP_T_CS16, fir = SDRHIP_FIR_CS16_EXACT }; typedef int16_t Real; };
template <> struct TypeTag<cf32> { enum { dtype = SDRHIP_T_CF32, fir = SDRHIP_FIR_CF32 }; typedef float Real; };
template <> struct TypeTag< std::complex<int8_t> > { enum { dtype = SDRHIP_T_CS8 }; typedef int8_t Real; };
template <> struct TypeTag< std::complex<double> > { enum { dtype = SDRHIP_T_CF64 }; typedef double Real; };

/** Owner of one handle of the C library: destroyed with its owner or when replaced, moved but never copied. */
template <class T, int (*Destroy)(T *)>
class Handle {
public:
  Handle() : _h(0) {}
  Handle(Handle &&o) noexcept : _h(o._h) { o._h = 0; }
  Handle &operator=(Handle &&o) noexcept { if (this != &o) { reset(); _h = o._h; o._h = 0; } return *this; }
  ~Handle() { reset(); }
  T *get() const { return _h; }
  operator T *() const { return _h; }   // (null while there is no plan: `if (_plan)`)
  void reset() { if (_h) { Destroy(_h); _h = 0; } }
  /** Where a create call stores its result; what was held before is destroyed first. */
  T **out() { reset(); return &_h; }
private:
  T *_h;
};
/** Owner of device memory; freed on the context it was allocated on. */
class DeviceMem {
public:
  DeviceMem() : _ctx(0), _p(0) {}
  DeviceMem(DeviceMem &&o) noexcept : _ctx(o._ctx), _p(o._p) { o._p = 0; }
  DeviceMem &operator=(DeviceMem &&o) noexcept { if (this != &o) { reset(); _ctx = o._ctx; _p = o._p; o._p = 0; } return *this; }
  ~DeviceMem() { reset(); }
  void alloc(sdrhip_ctx *c, size_t bytes, const char *what) { reset(); configCheck(sdrhip_malloc(c, bytes, &_p), what); _ctx = c; }
  void reset() { if (_p) { sdrhip_free(_ctx, _p); _p = 0; } }
  void *get() const { return _p; }
  template <class T> T *as() const { return static_cast<T *>(_p); }
private:
  sdrhip_ctx *_ctx;
  void *_p;
};
/** The registration of a host buffer as pinned memory (the buffer itself stays its node's). */
class Pinned {
public:
  Pinned() : _p(0) {}
  Pinned(const Pinned &) = delete;
  Pinned &operator=(const Pinned &) = delete;
  ~Pinned() { reset(); }
  void reset(void *p, size_t bytes, const char *what) { reset(); configCheck(sdrhip_host_register(p, bytes), what); _p = p; }
  void reset() { if (_p) { sdrhip_host_unregister(_p); _p = 0; } }
private:
  void *_p;
};

/** The designers' results as vectors. */
inline std::vector<int32_t> iqbbTaps(double Ff, double width, double Fs, size_t order) {
  std::vector<int32_t> taps(2 * order);
  design::iqbbTaps(Ff, width, Fs, order, taps.data());
  return taps;
}
inline std::vector<int32_t> freqShiftLut(bool int8 = false) {
  std::vector<int32_t> lut(2 * design::kLutSize);
  if (int8) design::freqShiftLutI8(lut.data()); else design::freqShiftLutI16(lut.data());
  return lut;
}
inline std::vector<double> firLowPass(size_t order, double Fu, double Fs) {
  std::vector<double> alpha(order);
  design::firLowPass(order, Fu, Fs, alpha.data());
  return alpha;
}
/** sinc_flt_kernel + FilterSource::_updateFilter (src/filternode.hh:18-28,186-203): the 2 x block-point spectrum of a band's kernel. */
template <class Scalar>
inline std::vector<Scalar> fftFilterSpectrum(size_t block, double fmin, double fmax, double Fs) {
  std::vector<Scalar> h(2 * block), K(4 * block);
  design::fftFilterKernel(int(block), fmin, fmax, Fs, h.data());
  design::fftFilterSpectrum(int(block), h.data(), K.data());
  return K;
}

/** The output of a baseband of complex COut with the demodulator `epilogue` fused into its launch: its sample type, and the
 * output elements per complex sample (the demodulators' int16 fits sizeof(COut) / 2 times into one). */
template <class COut> inline Config::Type fusedType(int epilogue) {
  return epilogue == SDRHIP_EPI_NONE ? Config::typeId<COut>() : Config::typeId<int16_t>();
}
template <class COut> inline size_t fusedPer(int epilogue) { return epilogue == SDRHIP_EPI_NONE ? 1 : sizeof(COut) / 2; }
/** The Config of every output of a bank: rows of `stride` at the decimated rate (int32 by size_t, as src/baseband.hh:192-193). */
inline Config bankOutConfig(int epilogue, int32_t Fs, size_t D, size_t stride) {
  return Config(fusedType<cs16>(epilogue), double(size_t(Fs) / D), stride, 1);
}
/** What such a baseband sends: the n samples at element `row` of `out`, as the nodes fused into it would have —
 * no demodulator: the complex view; FMDemod: int16, nothing for an empty buffer (src/demod.hh:231), overwrite not allowed;
 * AMDemod: int16, overwrite allowed (:80); USBDemod: int16, overwrite not allowed. `own`: the view is a buffer of its own
 * (a node's output); false for a row of a bank's shared staging buffer, which no receiver may write into. */
template <class COut>
inline void sendDemodulated(Source &from, int mode, const Buffer<COut> &out, size_t row, size_t n, bool own) {
  if (mode == SDRHIP_EPI_NONE) from.send(out.sub(row, n), own);
  else if (mode != SDRHIP_EPI_FM || n) from.send(Buffer<int16_t>(out).sub(row * (sizeof(COut) / 2), n), own && mode == SDRHIP_EPI_AM);
}

/** The direct hand-off of a result between two gpu nodes (detector -> BitStream: symbols; FilterSink -> FilterSource:
 * spectra): just before a direct send the producer records {host buffer data -> device copy, device}; the host buffer
 * stays unfilled, and a consumer that receives that very buffer reads the device copy. The keys are the addresses of live
 * host buffers, so one table serves all. Direct delivery is synchronous: the record lives as long as the send. */
struct Handoff { const void *dev; int device; };
inline std::map<const void *, Handoff> &handoffs() {
  static std::map<const void *, Handoff> table;
  return table;
}
class HandoffScope {
public:
  HandoffScope(const void *host, const void *dev, int device) : _host(host) { const Handoff rec = {dev, device}; handoffs()[host] = rec; }
  ~HandoffScope() { handoffs().erase(_host); }
  HandoffScope(const HandoffScope &) = delete;
private:
  const void *_host;
};
/** The device copy behind a received host buffer, or 0 when there is none on `device`. */
inline const void *handoffFor(const void *host, int device) {
  const std::map<const void *, Handoff>::const_iterator it = handoffs().find(host);
  return (it != handoffs().end() && it->second.device == device) ? it->second.dev : 0;
}
/** true: there are sinks, and every one is connected direct and is a SinkT on `device` (the condition of a hand-off). */
template <class SinkT>
inline bool allSinksDirectOn(const std::map<SinkBase *, bool> &sinks, int device) {
  if (sinks.empty()) return false;
  for (std::map<SinkBase *, bool>::const_iterator it = sinks.begin(); it != sinks.end(); ++it) {
    const SinkT *s = dynamic_cast<const SinkT *>(it->first);
    if (!it->second || !s || s->device() != device) return false;
  }
  return true;
}

// =================================================================================================
// the int16 baseband plans: IQBaseBand<int16_t|uint8_t|int8_t> and BaseBand<int16_t>
// =================================================================================================
/** One sdrhip_iqbb_i16 plan behind a node and what happens to it: made, retuned, reconfigured, run. The node says what
 * differs (_rate, _taps, _create) and keeps its parameters the way its reference node does. */
template <class In, class COut>
class Bb16 : public Sink<In>, public Source {
public:
  virtual ~Bb16() { _buffer.unref(); }
  /** Extension: fuse FMDemod / AMDemod / USBDemod<int16_t> (run in place on the node's output, as
   * `baseband.connect(&demod, true)` does in examples/sdr_fm.cc:51) into the same kernel launch.
   * The node then is a source of int16_t. Call before connecting / configuring. */
  void setDemod(int epilogue) { _epilogue = epilogue; if (_rate()) _reconfigure(); }

protected:
  Bb16(const char *name, double shift, size_t order, size_t sub_sample, int device)
    : _name(name), _gpuName(std::string("gpu::") + name), _shift(shift), _order(std::max(size_t(1), order)), _sub_sample(sub_sample),
      _sourceBs(0), _epilogue(SDRHIP_EPI_NONE), _device(device) {}

  virtual double _rate() const = 0;                    // the input sample rate as the node holds it; 0 before config()
  virtual std::vector<int32_t> _taps() const = 0;      // the filter kernel for the node's present parameters
  virtual int _create(const int32_t *taps, uint32_t inc, size_t D, sdrhip_iqbb_i16 **out) const = 0;
  virtual void _reconfigure() = 0;

  uint32_t _inc() const { return design::freqShiftIncrement(_shift, _rate()); }
  void _setShift() {
    if (_plan) configCheck(sdrhip_iqbb_i16_set_shift(_plan, _inc(), 0 > _shift), _name);
  }
  /** false: the new kernel does not fit the plan's formulation (tap bytes); a new plan has to take the stream over. */
  bool _setTaps() {
    const int rc = sdrhip_iqbb_i16_set_taps(_plan, _taps().data());
    if (rc == SDRHIP_E_UNSUPPORTED) return false;
    configCheck(rc, _name);
    return true;
  }
  /** _update_filter_kernel() on a configured node: swap the kernel, keep every bit of streaming state. */
  void _retap() {
    if (_plan && !_setTaps()) _newPlan(SDRHIP_KEEP_RING | SDRHIP_KEEP_FM | SDRHIP_KEEP_COUNTERS);
  }

  /** A device plan for the node's present parameters; `carry` (SDRHIP_KEEP_*) names the streaming state it takes over
   * from the plan it replaces (sdrhip_iqbb_i16_adopt_state), so that a new plan is not an event of its own. */
  void _newPlan(int carry) {
    const size_t D = std::max(size_t(1), _sub_sample);
    Handle<sdrhip_iqbb_i16, sdrhip_iqbb_i16_destroy> neu;
    configCheck(_create(_taps().data(), _inc(), D, neu.out()), _name);
    if (_plan) {
      if (_planOrder != _order) carry &= ~SDRHIP_KEEP_RING;   // (a new order is a new ring, src/baseband.hh:75-76)
      if (_planEpi != SDRHIP_EPI_FM || _epilogue != SDRHIP_EPI_FM) carry &= ~SDRHIP_KEEP_FM;
      configCheck(sdrhip_iqbb_i16_adopt_state(neu, _plan, carry), _name);
    }
    _plan = std::move(neu);
    _planOrder = _order; _planD = D; _planBs = _sourceBs; _planEpi = _epilogue;
  }

  /** IQBaseBand::_reconfigure (src/baseband.hh:156-194) and BaseBand::config (:357-395): kernel and LUT increment
   * recomputed, counters and phases reset, the FIR ring's CONTENTS kept where they lie (read rotated afterwards) — on the
   * plan in place (sdrhip_iqbb_i16_reset(keep_history = 1)) or, when the geometry changed (order, decimation, buffer size,
   * demodulator), carried into the new device plan. Returns the Config to propagate, over a new output buffer. */
  Config _configure(size_t D, double oRate) {
    size_t buffer_size = _sourceBs / D;
    if (_sourceBs % D) buffer_size += 1;
    const Config out_cfg(fusedType<COut>(_epilogue), oRate, buffer_size, 1);
    // (a fused demodulator is reconfigured — FM's last angle zeroed — only if the Config we propagate changes,
    // src/node.cc:98-105, src/demod.hh:210)
    const bool same_cfg = (out_cfg == this->_config);
    if (_plan && _planOrder == _order && _planD == D && _planBs == _sourceBs && _planEpi == _epilogue && _setTaps()) {
      _setShift();
      configCheck(sdrhip_iqbb_i16_reset(_plan, same_cfg ? 3 : 1), _name);
    } else _newPlan(SDRHIP_KEEP_RING | (same_cfg ? SDRHIP_KEEP_FM : 0));
    _buffer.unref();
    _buffer = Buffer<COut>(buffer_size);
    return out_cfg;
  }

  void _run(const Buffer<In> &in, const Buffer<COut> &out) {
    size_t n = 0;
    // (out_stride in output elements)
    if (!processOk(sdrhip_iqbb_i16_process(_plan, reinterpret_cast<const int16_t *>(in.data()), in.size(), 0, out.data(),
                                           out.size() * fusedPer<COut>(_epilogue), &n), _gpuName.c_str()))
      return;
    sendDemodulated(*this, _epilogue, out, 0, n, true);
  }

  const char *_name;
  std::string _gpuName;
  double _shift;
  size_t _order, _sub_sample, _sourceBs;
  int _epilogue, _device;
  Handle<sdrhip_iqbb_i16, sdrhip_iqbb_i16_destroy> _plan;
  size_t _planOrder = 0, _planD = 0, _planBs = 0;   // geometry the device plan was made for
  int _planEpi = 0;
  Buffer<COut> _buffer;
};

/** Sample types per input scalar: int16_t and uint8_t (AutoCast fused) produce complex<int16_t>; int8_t is
 * IQBaseBand<int8_t>, which produces complex<int8_t> (reference src/baseband.hh:22-31, src/sdr.hh:225-240). */
template <class S> struct BbIo { typedef cs16 COut; enum { int8 = 0, cu8 = 0 }; };
template <> struct BbIo<uint8_t> { typedef cs16 COut; enum { int8 = 0, cu8 = 1 }; };
template <> struct BbIo<int8_t> { typedef std::complex<int8_t> COut; enum { int8 = 1, cu8 = 0 }; };

/** IQBaseBand on the int16 kernels; SIn = int16_t (complex<int16_t> in) or uint8_t (complex<uint8_t> in, with
 * AutoCast< complex<int16_t> > fused into the load: the cast -> baseband pair of examples/sdr_fm.cc:49-50). */
template <class SIn>
class IQBB16 : public Bb16< std::complex<SIn>, typename BbIo<SIn>::COut > {
public:
  typedef std::complex<SIn> CIn;
  typedef typename BbIo<SIn>::COut COut;
  enum { kInt8 = BbIo<SIn>::int8, kCu8 = BbIo<SIn>::cu8 };
  IQBB16(double Fc, double width, size_t order, size_t sub_sample, double oFs = 0.0, int device = 0)
    : IQBB16(Fc, Fc, width, order, sub_sample, oFs, device) {}
  IQBB16(double Fc, double Ff, double width, size_t order, size_t sub_sample, double oFs = 0.0, int device = 0)
    : Bb16<CIn, COut>("IQBaseBand", Fc, order, sub_sample, device), _Fc(Fc), _Ff(Ff), _Fs(0), _width(width), _oFs(oFs) {}

  inline size_t order() const { return this->_order; }
  /** As the reference (src/baseband.hh:69-79): a new kernel and a NEW ring; the decimator window, the sample counter, the
   * LUT phase and the Config go on untouched. (The reference's new ring is uninitialised memory until `order` samples
   * have passed; here it is zeros.) */
  void setOrder(size_t o) {
    this->_order = std::max(size_t(1), o);
    if (this->_plan) this->_newPlan(SDRHIP_KEEP_FM | SDRHIP_KEEP_COUNTERS);
  }
  inline double centerFrequency() const { return _Fc; }
  /** As the reference (src/baseband.hh:84-86 -> src/freqshift.hh:52-54,78-87): new LUT increment and sign, the LUT
   * phase restarts; filter history, decimator state and the kernel go on unchanged. */
  void setCenterFrequency(double Fc) { _Fc = int32_t(Fc); this->_shift = _Fc; this->_setShift(); }
  inline double filterFrequency() const { return _Ff; }
  /** As the reference (:92-104): only the filter kernel is recomputed, all streaming state goes on. */
  void setFilterFrequency(double Ff) { _Ff = int32_t(Ff); this->_retap(); }
  inline double filterWidth() const { return _width; }
  void setFilterWidth(double width) { _width = int32_t(width); this->_retap(); }
  size_t subSample() const { return this->_sub_sample; }
  void setSubsample(size_t sub_sample) { this->_sub_sample = std::max(size_t(1), sub_sample); if (_Fs) _reconfigure(); }
  void setOutputSampleRate(double Fs) { _oFs = Fs; if (_Fs) _reconfigure(); }

  virtual void config(const Config &src_cfg) {
    if (!src_cfg.hasType() || !src_cfg.hasSampleRate() || !src_cfg.hasBufferSize()) return;
    checkType<CIn>(src_cfg, "IQBaseBand");
    _Fs = int32_t(src_cfg.sampleRate());
    this->_sourceBs = src_cfg.bufferSize();
    _reconfigure();
  }

  virtual void process(const Buffer<CIn> &buffer, bool allow_overwrite) {
    if (!this->_plan) return;
    if (allow_overwrite && sizeof(CIn) == sizeof(COut)) this->_run(buffer, Buffer<COut>(buffer));   // in place needs equal sample sizes
    else if (this->_buffer.isUnused()) this->_run(buffer, this->_buffer);
    // else: output buffer still in use downstream -> the input is dropped (src/baseband.hh:141-150)
  }

protected:
  virtual double _rate() const { return double(_Fs); }
  virtual std::vector<int32_t> _taps() const { return iqbbTaps(_Ff, _width, _Fs, this->_order); }
  virtual int _create(const int32_t *taps, uint32_t inc, size_t D, sdrhip_iqbb_i16 **out) const {
    int rc = (kInt8 ? sdrhip_iqbb_i8_create : sdrhip_iqbb_i16_create)(Device::get(this->_device), taps, int(this->_order),
                 freqShiftLut(kInt8).data(), inc, 0 > this->_shift, int(D), 1, this->_sourceBs, this->_epilogue, out);
    if (rc == SDRHIP_OK && kCu8) rc = sdrhip_iqbb_i16_set_input_format(*out, SDRHIP_IN_CU8);
    return rc;
  }
  /** The decimation follows the output rate, where one is given, and is written back (src/baseband.hh:159-162). */
  virtual void _reconfigure() {
    const size_t D = design::iqbbDecimation(_Fs, this->_sub_sample, _oFs);
    this->_sub_sample = D;
    // the reference divides int32 by size_t (src/baseband.hh:192-193)
    const Config out_cfg = this->_configure(D, double(size_t(_Fs) / D));

    LogMessage msg(LOG_DEBUG);
    msg << "Configured gpu::IQBaseBand node:" << std::endl << " sample-rate " << _Fs << "Hz" << std::endl
        << " center freq " << _Fc << "Hz" << std::endl << " width " << _width << "Hz" << std::endl
        << " in buffer size " << this->_sourceBs << std::endl << " sub-sample by " << D << std::endl
        << " out buffer size " << out_cfg.bufferSize();
    Logger::get().log(msg);

    this->setConfig(out_cfg);
  }

  // as the reference node keeps them (src/baseband.hh:266-272): int32 members, truncated; only the frequency shift
  // (Bb16::_shift) starts as the constructor's untruncated double
  int32_t _Fc, _Ff, _Fs, _width;
  double _oFs;
};
}  // namespace detail

template <class Scalar> class IQBaseBand;
/** Drop-in for sdr::IQBaseBand<int16_t>. */
template <>
class IQBaseBand<int16_t> : public detail::IQBB16<int16_t> {
public:
  using detail::IQBB16<int16_t>::IQBB16;
};
/** Drop-in for sdr::IQBaseBand<int8_t>, the baseband of the reference's documentation example (src/sdr.hh:225-240):
 * sinks and sources complex<int8_t>. */
template <>
class IQBaseBand<int8_t> : public detail::IQBB16<int8_t> {
public:
  using detail::IQBB16<int8_t>::IQBB16;
};
/** AutoCast< complex<int16_t> > + IQBaseBand<int16_t> in one node: sinks complex<uint8_t> (RTL-SDR bytes). */
template <>
class IQBaseBand<uint8_t> : public detail::IQBB16<uint8_t> {
public:
  using detail::IQBB16<uint8_t>::IQBB16;
};

/** IQBaseBand<float> — BASELINE config 2's node. The reference has NO working float baseband (IQBaseBand<float> does not
 * compile: its compute type is hard-wired to int32, src/baseband.hh:28-31,205; FreqShift<float> truncates every sample to
 * int16), so this node is BUILD-DEFINED behind the reference's constructor signatures
 * (src/baseband.hh:33-37) and its config / ownership / drop rules (:115-151):
 *     y = SubSample_D( FIRLowPass_cf32( x[n] * exp(-2*pi*i*Fc*n/Fs) ) ),   low-pass cut-off = width / 2
 * — the band of `width` Hz around Fc moved to 0 Hz, filtered with FIRLowPassCoeffs (src/firfilter.hh:16-32: the
 * reference's own cf32 arithmetic, pinned) and box-averaged like SubSample<complex<float>> (src/subsample.hh:92-101:
 * pinned); the phasor is the float64 closed form of the absolute sample index (parity unpinned by necessity, checked
 * against that closed form, <= 1e-5). A filter frequency other than Fc would need complex taps this definition does not
 * have: it is refused with a ConfigError rather than silently filtered around the wrong centre. D = Fs / oFs when an
 * output rate is given, as the reference node (:159-162). Never in place (the output is D times shorter and the node
 * owns it); the input is dropped while the output buffer is still referenced downstream (:141-150). */
template <>
class IQBaseBand<float> : public Sink<cf32>, public Source {
public:
  IQBaseBand(double Fc, double width, size_t order, size_t sub_sample, double oFs = 0.0, int device = 0)
    : IQBaseBand(Fc, Fc, width, order, sub_sample, oFs, device) {}
  IQBaseBand(double Fc, double Ff, double width, size_t order, size_t sub_sample, double oFs = 0.0, int device = 0)
    : _Fc(Fc), _Ff(Ff), _width(width), _Fs(0), _order(std::max(size_t(1), order)), _sub_sample(std::max(size_t(1), sub_sample)),
      _oFs(oFs), _sourceBs(0), _device(device) {}
  virtual ~IQBaseBand() { _buffer.unref(); }
  inline size_t order() const { return _order; }
  /** A new order is a new plan (filter history, decimator and phasor restart: the reference's setOrder reallocates its ring
   * too, src/baseband.hh:69-79); the same order changes nothing. */
  void setOrder(size_t o) { o = std::max(size_t(1), o); if (o == _order) return; _order = o; if (_Fs) _reconfigure(); }
  inline double centerFrequency() const { return _Fc; }
  /** The plan and its streaming state are KEPT (src/baseband.hh:82-86: setCenterFrequency only updates the LUT increment):
   * the phasor restarts at the current sample with the new frequency, filter history and decimator go on.
   * The build-defined float baseband filters AROUND its centre frequency (class comment): the centre takes the filter
   * frequency with it, so that a retune is one call and never passes through an unsupported (Fc, Ff) pair. */
  void setCenterFrequency(double Fc) {
    _Fc = Fc; _Ff = Fc;
    if (_plan) detail::configCheck(sdrhip_fbb_f32_set_shift(_plan, _Fc), "IQBaseBand<float>");
    else if (_Fs) _reconfigure();
  }
  inline double filterFrequency() const { return _Ff; }
  /** Checked BEFORE anything changes: on a configured node a filter frequency other than the centre frequency throws
   * ConfigError and leaves the node as it was (same values, same plan). */
  void setFilterFrequency(double Ff) {
    if (_Fs && Ff != _Fc) {
      ConfigError err;
      err << "Can not set filter frequency " << Ff << "Hz on IQBaseBand<float>: it differs from the center frequency " << _Fc
          << "Hz (the build-defined float baseband low-pass filters the shifted band: sdr/gpu/nodes.hh); the node is unchanged";
      throw err;
    }
    _Ff = Ff;   // (equal to the centre frequency: nothing to update)
    if (_Fs && !_plan) _reconfigure();
  }
  inline double filterWidth() const { return _width; }
  /** New coefficients on the SAME plan (src/baseband.hh:95-101: setFilterWidth only recomputes the kernel; the ring stays). */
  void setFilterWidth(double width) {
    _width = width;
    if (_plan) detail::configCheck(sdrhip_fbb_f32_set_taps(_plan, detail::firLowPass(_order, _width / 2, _Fs).data()), "IQBaseBand<float>");
    else if (_Fs) _reconfigure();
  }
  size_t subSample() const { return _sub_sample; }
  /** A decimation that does not change keeps plan and state; a new one is a new plan (the reference runs _reconfigure:
   * counters reset, src/baseband.hh:106-112). */
  void setSubsample(size_t sub_sample) {
    sub_sample = std::max(size_t(1), sub_sample);
    const bool same = _plan && _oFs <= 0 && sub_sample == _sub_sample;
    _sub_sample = sub_sample;
    if (_Fs && !same) _reconfigure();
  }
  void setOutputSampleRate(double Fs) {
    const bool same = _plan && Fs > 0 && design::iqbbDecimation(_Fs, _sub_sample, Fs) == _sub_sample;
    _oFs = Fs;
    if (_Fs && !same) _reconfigure();
  }

  virtual void config(const Config &src_cfg) {
    if (!src_cfg.hasType() || !src_cfg.hasSampleRate() || !src_cfg.hasBufferSize()) return;
    detail::checkType<cf32>(src_cfg, "IQBaseBand");
    _Fs = src_cfg.sampleRate();
    _sourceBs = src_cfg.bufferSize();
    _reconfigure();
  }

  virtual void process(const Buffer<cf32> &buffer, bool allow_overwrite) {
    (void)allow_overwrite;
    if (!_plan) return;
    if (!_buffer.isUnused()) return;   // output still in use downstream: the input is dropped (src/baseband.hh:141-150)
    size_t n = 0;
    if (!detail::processOk(sdrhip_fbb_f32_process(_plan, reinterpret_cast<const float *>(buffer.data()), buffer.size(), 0,
                                                  reinterpret_cast<float *>(_buffer.data()), _buffer.size(), &n), "gpu::IQBaseBand<float>"))
      return;
    this->send(_buffer.head(n), true);
  }

protected:
  void _reconfigure() {
    if (_Ff != _Fc) {
      ConfigError err;
      err << "Can not configure IQBaseBand<float>: filter frequency " << _Ff << "Hz differs from the center frequency " << _Fc
          << "Hz (the build-defined float baseband low-pass filters the shifted band: sdr/gpu/nodes.hh)";
      throw err;
    }
    const size_t D = design::iqbbDecimation(_Fs, _sub_sample, _oFs);
    _sub_sample = D;
    const std::vector<double> alpha = detail::firLowPass(_order, _width / 2, _Fs);
    detail::configCheck(sdrhip_fbb_f32_create(Device::get(_device), _Fc, _Fs, alpha.data(), int(_order), int(D), 1, _sourceBs, _plan.out()),
                        "IQBaseBand<float>");
    size_t buffer_size = _sourceBs / D + 1;   // (a call may emit one output more than Bs / D: the decimator's phase carries over)
    _buffer.unref();
    _buffer = Buffer<cf32>(buffer_size);
    LogMessage msg(LOG_DEBUG);
    msg << "Configured gpu::IQBaseBand<float> node:" << std::endl << " sample-rate " << _Fs << "Hz" << std::endl
        << " center freq " << _Fc << "Hz" << std::endl << " width " << _width << "Hz" << std::endl
        << " in buffer size " << _sourceBs << std::endl << " sub-sample by " << D << std::endl
        << " out buffer size " << buffer_size;
    Logger::get().log(msg);
    this->setConfig(Config(Config::typeId<cf32>(), _Fs / double(D), buffer_size, 1));
  }

  double _Fc, _Ff, _width, _Fs;
  size_t _order, _sub_sample;
  double _oFs;
  size_t _sourceBs;
  int _device;
  detail::Handle<sdrhip_fbb_f32, sdrhip_fbb_f32_destroy> _plan;
  Buffer<cf32> _buffer;
};

// =================================================================================================
// BaseBand<int16_t>: the REAL-input baseband node (reference src/baseband.hh:305-529)
// =================================================================================================
template <class Scalar> class BaseBand;
/** Drop-in for sdr::BaseBand<int16_t>: sinks int16_t, sources complex<int16_t> at Fs/sub_sample. Never works in
 * place (the reference's process() ignores allow_overwrite, :408-419); drops the input while the output buffer is
 * still in use downstream. */
template <>
class BaseBand<int16_t> : public detail::Bb16<int16_t, cs16> {
public:
  BaseBand(double Fc, double width, size_t order, size_t sub_sample) : BaseBand(Fc, Fc, width, order, sub_sample, 0) {}
  BaseBand(double Fc, double Ff, double width, size_t order, size_t sub_sample, int device = 0)
    : detail::Bb16<int16_t, cs16>("BaseBand", Fc, order, sub_sample, device), _Ff(Ff), _width(width), _Fs(0) {}
  inline double sampleRate() const { return _Fs; }
  inline double frequencyShift() const { return _shift; }
  /** FreqShiftBase::setFrequencyShift (src/freqshift.hh:52-54,78-87): new increment and sign, the LUT phase restarts;
   * ring, decimator and kernel go on. */
  void setFrequencyShift(double F) { _shift = F; _setShift(); }
  /** BaseBand::setSampleRate (src/baseband.hh:397-401): the LUT increment and the kernel are recomputed, nothing is
   * propagated (the reference marks that as a bug of its own, :400). */
  void setSampleRate(double Fs) { _Fs = Fs; _setShift(); _retap(); }

  virtual void config(const Config &src_cfg) {
    if (!src_cfg.hasType() || !src_cfg.hasSampleRate() || !src_cfg.hasBufferSize()) return;
    detail::checkType<int16_t>(src_cfg, "BaseBand");
    _Fs = src_cfg.sampleRate();
    _sourceBs = src_cfg.bufferSize();
    _reconfigure();
  }

  virtual void process(const Buffer<int16_t> &buffer, bool allow_overwrite) {
    (void)allow_overwrite;
    if (_plan && _buffer.isUnused()) _run(buffer, _buffer);
  }

protected:
  virtual double _rate() const { return _Fs; }
  virtual std::vector<int32_t> _taps() const {
    std::vector<int32_t> taps(2 * _order);
    design::bbTaps(_Ff, _width, _Fs, _order, taps.data());
    return taps;
  }
  virtual int _create(const int32_t *taps, uint32_t inc, size_t D, sdrhip_iqbb_i16 **out) const {
    return sdrhip_bb_i16_create(Device::get(_device), taps, int(_order), detail::freqShiftLut().data(), inc, 0 > _shift, int(D), 1,
                                _sourceBs, _epilogue, out);
  }
  /** The decimation is the constructor's; the output rate is the double quotient (src/baseband.hh:357-395). */
  virtual void _reconfigure() { this->setConfig(_configure(_sub_sample, _Fs / _sub_sample)); }

  double _Ff, _width, _Fs;
};

// =================================================================================================
// FIRLowPass<complex<int16_t>> (bit-exact) / FIRLowPass<complex<float>>
// =================================================================================================
template <class Scalar>
class FIRLowPass : public Sink<Scalar>, public Source {
public:
  FIRLowPass(size_t order, double Fc, int device = 0)
    : _enabled(true), _order(std::max(size_t(1), order)), _Fu(Fc), _Fs(0), _bs(0), _device(device) {}
  virtual ~FIRLowPass() { _buffer.unref(); }
  inline bool enabled() const { return _enabled; }
  inline void enable(bool enable) { _enabled = enable; }
  inline size_t order() const { return _order; }
  virtual void setOrder(size_t order) { order = std::max(size_t(1), order); if (order == _order) return; _order = order; if (_Fs) _plan_(); }
  inline double freq() const { return _Fu; }
  /** FIRFilter::setUpperFreq (src/firfilter.hh:165-170,287): only the coefficients change; the ring — the stream — goes on. */
  inline void setFreq(double freq) {
    _Fu = freq;
    if (!_Fs) return;
    if (!_plan) { _plan_(); return; }
    detail::configCheck(sdrhip_fir_set_taps(_plan, detail::firLowPass(_order, _Fu, _Fs).data()), "FIRLowPass");
  }

  virtual void config(const Config &src_cfg) {
    if (!src_cfg.hasType() || !src_cfg.hasSampleRate() || !src_cfg.hasBufferSize()) return;
    detail::checkType<Scalar>(src_cfg, "FIRLowPass");
    _Fs = src_cfg.sampleRate();
    _bs = src_cfg.bufferSize();
    _plan_();   // a fresh plan = zeroed ring, as FIRFilter::config does (src/firfilter.hh:193-195)
    if (!_buffer.isEmpty()) _buffer.unref();
    _buffer = Buffer<Scalar>(_bs);
    this->setConfig(Config(src_cfg.type(), src_cfg.sampleRate(), src_cfg.bufferSize(), 1));
  }

  virtual void process(const Buffer<Scalar> &buffer, bool allow_overwrite) {
    if (!_enabled) { this->send(buffer, allow_overwrite); return; }
    if (!_plan) return;
    if (allow_overwrite) _process(buffer, buffer);
    else if (_buffer.isUnused()) _process(buffer, _buffer);
  }

protected:
  void _plan_() {
    const std::vector<double> alpha = detail::firLowPass(_order, _Fu, _Fs);
    detail::configCheck(sdrhip_fir_create(Device::get(_device), detail::TypeTag<Scalar>::fir, alpha.data(), int(_order), 1, 1,
                                          _bs, SDRHIP_EPI_NONE, _plan.out()), "FIRLowPass");
  }
  void _process(const Buffer<Scalar> &in, const Buffer<Scalar> &out) {
    size_t n = 0;
    if (!detail::processOk(sdrhip_fir_process(_plan, in.data(), in.size(), 0, out.data(), out.size(), &n), "gpu::FIRLowPass")) return;
    this->send(out.head(in.size()), true);
  }
  bool _enabled;
  size_t _order;
  double _Fu, _Fs;
  size_t _bs;
  int _device;
  detail::Handle<sdrhip_fir, sdrhip_fir_destroy> _plan;
  Buffer<Scalar> _buffer;
};

// =================================================================================================
// demodulators
// =================================================================================================
namespace detail {
template <class InC, class OutR>
class DemodBase : public Sink<InC>, public Source {
public:
  DemodBase(int kind, const char *name, int device) : _kind(kind), _name(name), _device(device), _can_overwrite(true) {}
  virtual ~DemodBase() { _buffer.unref(); }
  virtual void config(const Config &src_cfg) {
    if (!src_cfg.hasType() || !src_cfg.hasBufferSize()) return;
    checkType<InC>(src_cfg, _name);
    configCheck(sdrhip_demod_create(Device::get(_device), _kind, TypeTag<InC>::dtype, 1, src_cfg.bufferSize(), 0, _plan.out()), _name);
    if (!_buffer.isEmpty()) _buffer.unref();
    _buffer = Buffer<OutR>(src_cfg.bufferSize());
    this->setConfig(Config(Config::typeId<OutR>(), src_cfg.sampleRate(), src_cfg.bufferSize(),
                           _kind == SDRHIP_EPI_AM ? src_cfg.numBuffers() : 1));
  }
  virtual void process(const Buffer<InC> &buffer, bool allow_overwrite) {
    if (!_plan) return;
    if (_kind == SDRHIP_EPI_FM && 0 == buffer.size()) return;            // src/demod.hh:231
    Buffer<OutR> out = (allow_overwrite && _can_overwrite) ? Buffer<OutR>(buffer) : _buffer;
    // in place the output aliases the input bytes, so FM's untouched out[0] is in[0].real()
    if (!processOk(sdrhip_demod_process(_plan, buffer.data(), buffer.size(), 0, out.data(), 0), _name)) return;
    this->send(out.head(buffer.size()), _kind == SDRHIP_EPI_AM);        // AM sends with allow_overwrite=true (:80)
  }

protected:
  int _kind;
  const char *_name;
  int _device;
  Handle<sdrhip_demod, sdrhip_demod_destroy> _plan;
  bool _can_overwrite;
  Buffer<OutR> _buffer;
};
}  // namespace detail

template <class iScalar, class oScalar = iScalar> class FMDemod;
template <>
class FMDemod<int16_t, int16_t> : public detail::DemodBase<cs16, int16_t> {
public:
  explicit FMDemod(int device = 0) : detail::DemodBase<cs16, int16_t>(SDRHIP_EPI_FM, "FMDemod", device) {}
};
/** FMDemod<int8_t,int16_t> (reference src/demod.hh:173-262 with src/math.hh:12-21): complex<int8_t> in, int16_t out,
 * in place when allowed (an output element covers exactly its input sample). */
template <>
class FMDemod<int8_t, int16_t> : public detail::DemodBase<std::complex<int8_t>, int16_t> {
public:
  explicit FMDemod(int device = 0) : detail::DemodBase<std::complex<int8_t>, int16_t>(SDRHIP_EPI_FM, "FMDemod", device) {}
};
template <class Scalar>
class AMDemod : public detail::DemodBase<std::complex<Scalar>, Scalar> {
public:
  explicit AMDemod(int device = 0) : detail::DemodBase<std::complex<Scalar>, Scalar>(SDRHIP_EPI_AM, "AMDemod", device) {}
};
template <class Scalar>
class USBDemod : public detail::DemodBase<std::complex<Scalar>, Scalar> {
public:
  explicit USBDemod(int device = 0) : detail::DemodBase<std::complex<Scalar>, Scalar>(SDRHIP_EPI_USB, "USBDemod", device) {}
};

/** FMDeemph<int16_t> (reference src/demod.hh:272-362). */
template <class Scalar> class FMDeemph;
template <>
class FMDeemph<int16_t> : public Sink<int16_t>, public Source {
public:
  explicit FMDeemph(bool enabled = true, int device = 0) : _enabled(enabled), _device(device) {}
  virtual ~FMDeemph() { _buffer.unref(); }
  inline bool isEnabled() const { return _enabled; }
  inline void enable(bool enabled) { _enabled = enabled; }
  virtual void config(const Config &src_cfg) {
    if (!src_cfg.hasType() || !src_cfg.hasSampleRate() || !src_cfg.hasBufferSize()) return;
    detail::checkType<int16_t>(src_cfg, "FMDeemph");
    _plan.reset();   // a fresh plan: average reset to 0 (:308)
    detail::configCheck(sdrhip_deemph_i16_create(Device::get(_device), design::fmDeemphAlpha(src_cfg.sampleRate()), 1,
                                                 src_cfg.bufferSize(), _plan.out()), "FMDeemph");
    _buffer.unref();
    _buffer = Buffer<int16_t>(src_cfg.bufferSize());
    this->setConfig(Config(src_cfg.type(), src_cfg.sampleRate(), src_cfg.bufferSize(), 1));
  }
  virtual void process(const Buffer<int16_t> &buffer, bool allow_overwrite) {
    if (!_enabled) { this->send(buffer, allow_overwrite); return; }
    if (!_plan) return;
    const Buffer<int16_t> &out = allow_overwrite ? buffer : _buffer;
    if (!detail::processOk(sdrhip_deemph_i16_process(_plan, reinterpret_cast<const int16_t *>(buffer.data()), buffer.size(), 0,
                                                     reinterpret_cast<int16_t *>(out.data()), 0), "gpu::FMDeemph")) return;
    if (allow_overwrite) this->send(buffer, allow_overwrite);
    else this->send(_buffer.head(buffer.size()), false);
  }

protected:
  bool _enabled;
  int _device;
  detail::Handle<sdrhip_deemph, sdrhip_deemph_i16_destroy> _plan;
  Buffer<int16_t> _buffer;
};

// =================================================================================================
// audio to bits: FSKDetector, ASKDetector<int16_t>, BitStream (reference src/fsk.hh, src/fsk.cc)
// =================================================================================================
/** Drop-in for sdr::BitStream (reference src/fsk.hh:124-171, src/fsk.cc:102-202): symbols in, bits out, sent only when a
 * buffer produced at least one (:201). The output buffer holds ceil(bufferSize * omegaMax) + 1 bits (the reference's
 * 1 + bufferSize / corrLen can be exceeded by its own PLL); the Config forwarded says so. */
class BitStream : public Sink<uint8_t>, public Source {
public:
  typedef enum { NORMAL, TRANSITION } Mode;
  explicit BitStream(float baud, Mode mode = TRANSITION, int device = 0)
    : _baud(baud), _mode(mode), _device(device), _cap(0), _onDevice(false) {}
  virtual ~BitStream() { _buffer.unref(); }
  virtual void config(const Config &src_cfg) {
    if (!src_cfg.hasType() || !src_cfg.hasSampleRate()) return;
    // (the type named as expected is the reference's, src/fsk.cc:116)
    detail::checkType(src_cfg, Config::typeId<uint8_t>(), Config::typeId<int16_t>(), "BitStream");
    _plan.reset();   // a fresh plan: ring, PLL and bit history start over (:125-140)
    sdrhip_ctx *c = Device::get(_device);
    const size_t bs = std::max(size_t(1), src_cfg.bufferSize());
    detail::configCheck(sdrhip_bits_create(c, src_cfg.sampleRate(), _baud, _mode == TRANSITION ? SDRHIP_BITS_TRANSITION : SDRHIP_BITS_NORMAL,
                                           1, bs, _plan.out()), "BitStream");
    detail::configCheck(sdrhip_bits_out_capacity(_plan, bs, &_cap), "BitStream");
    _in.alloc(c, bs, "BitStream");
    _out.alloc(c, _cap, "BitStream");
    _counts.alloc(c, sizeof(uint32_t), "BitStream");
    _buffer.unref();
    _buffer = Buffer<uint8_t>(_cap);
    LogMessage msg(LOG_DEBUG);
    msg << "Config BitStream node: " << std::endl
        << " symbol rate: " << src_cfg.sampleRate() << " Hz" << std::endl
        << " baud rate:   " << _baud << std::endl
        << " symbols/bit: " << 1. / float(_baud / src_cfg.sampleRate()) << std::endl
        << " bit mode:    " << ((NORMAL == _mode) ? "normal" : "transition");
    Logger::get().log(msg);
    this->setConfig(Config(Config::typeId<uint8_t>(), _baud, _buffer.size(), 1));   // :154
  }
  virtual void process(const Buffer<uint8_t> &buffer, bool) {
    if (!_plan) return;
    sdrhip_ctx *c = Device::get(_device);
    const void *handed = detail::handoffFor(buffer.data(), _device);
    _onDevice = handed != 0;
    const uint8_t *sym = _onDevice ? static_cast<const uint8_t *>(handed) : _in.as<uint8_t>();
    if (!_onDevice && buffer.size() &&
        !detail::processOk(sdrhip_memcpy_h2d(c, _in.get(), buffer.data(), buffer.size()), "gpu::BitStream")) return;
    if (!detail::processOk(sdrhip_bits_process_dev(_plan, sym, buffer.size(), 0, _out.as<uint8_t>(), _cap, _counts.as<uint32_t>()),
                           "gpu::BitStream")) return;
    uint32_t o = 0;
    if (!detail::processOk(sdrhip_memcpy_d2h(c, &o, _counts.get(), sizeof(o)), "gpu::BitStream")) return;
    if (0 == o) return;                                                              // :201
    if (!_buffer.isUnused()) return;   // still referenced downstream: the bits of this buffer are dropped
    if (!detail::processOk(sdrhip_memcpy_d2h(c, _buffer.data(), _out.get(), o), "gpu::BitStream")) return;
    this->send(_buffer.head(o));
  }
  /** true: the last buffer's symbols were read from a gpu detector's device memory (no host copy in between). */
  bool lastBufferOnDevice() const { return _onDevice; }
  int device() const { return _device; }

protected:
  float _baud;
  Mode _mode;
  int _device;
  detail::Handle<sdrhip_bits, sdrhip_bits_destroy> _plan;
  detail::DeviceMem _in, _out, _counts;
  size_t _cap;
  bool _onDevice;
  Buffer<uint8_t> _buffer;
};

namespace detail {
/** What FSKDetector and ASKDetector share: int16 in, one symbol per sample out, sent as head(n) with overwrite disallowed
 * (reference src/fsk.cc:94, src/fsk.hh:110). When every connected sink is connected direct and is a gpu::BitStream on the
 * same device, the symbols stay on the device and the buffer sent is left unfilled; otherwise they are copied into it. */
class DetectorBase : public Sink<int16_t>, public Source {
public:
  DetectorBase(const char *name, int device) : _name(name), _device(device), _onDevice(false) {}
  virtual ~DetectorBase() { _buffer.unref(); }
  virtual void process(const Buffer<int16_t> &buffer, bool) {
    if (!_plan) return;
    sdrhip_ctx *c = Device::get(_device);
    const size_t n = buffer.size();
    if (n && (!processOk(sdrhip_memcpy_h2d(c, _in.get(), buffer.data(), n * sizeof(int16_t)), _name) ||
              !processOk(sdrhip_detector_process_dev(_plan, _in.as<int16_t>(), n, 0, _sym.as<uint8_t>(), 0), _name))) return;
    _onDevice = allSinksDirectOn<gpu::BitStream>(_sinks, _device);
    if (!_onDevice) {
      if (n && !processOk(sdrhip_memcpy_d2h(c, _buffer.data(), _sym.get(), n), _name)) return;
      this->send(_buffer.head(n), false);
      return;
    }
    const HandoffScope handoff(_buffer.data(), _sym.get(), _device);
    this->send(_buffer.head(n), false);
  }
  /** true: the last buffer's symbols went to the BitStream nodes on the device (no host copy). */
  bool lastBufferOnDevice() const { return _onDevice; }

protected:
  void _plan_(int kind, const float *mark, const float *space, int corrLen, bool invert, size_t bufferSize) {
    sdrhip_ctx *c = Device::get(_device);
    const size_t bs = std::max(size_t(1), bufferSize);
    configCheck(sdrhip_detector_create(c, kind, mark, space, corrLen, invert ? 1 : 0, 1, bs, _plan.out()), _name);
    _in.alloc(c, bs * sizeof(int16_t), _name);
    _sym.alloc(c, bs, _name);
    _buffer.unref();
    _buffer = Buffer<uint8_t>(bs);
  }
  const char *_name;
  int _device;
  Handle<sdrhip_detector, sdrhip_detector_destroy> _plan;
  DeviceMem _in, _sym;
  bool _onDevice;
  Buffer<uint8_t> _buffer;
};
}  // namespace detail

/** Drop-in for sdr::FSKDetector (reference src/fsk.hh:18-56, src/fsk.cc:12-95). */
class FSKDetector : public detail::DetectorBase {
public:
  FSKDetector(float baud, float Fmark, float Fspace, int device = 0)
    : detail::DetectorBase("FSKDetector", device), _baud(baud), _corrLen(0), _Fmark(Fmark), _Fspace(Fspace) {}
  virtual void config(const Config &src_cfg) {
    if (!src_cfg.hasType() || !src_cfg.hasSampleRate()) return;
    detail::checkType<int16_t>(src_cfg, "FSKBase");
    _corrLen = size_t(design::fskCorrLen(src_cfg.sampleRate(), _baud));
    std::vector<float> mark(2 * _corrLen), space(2 * _corrLen);
    design::fskLut(src_cfg.sampleRate(), _Fmark, int(_corrLen), mark.data());
    design::fskLut(src_cfg.sampleRate(), _Fspace, int(_corrLen), space.data());
    _plan_(SDRHIP_DET_FSK, mark.data(), space.data(), int(_corrLen), false, src_cfg.bufferSize());   // rings zeroed, index 0 (:48-51)
    LogMessage msg(LOG_DEBUG);
    msg << "Config FSKDetector node: " << std::endl
        << " sample/symbol rate: " << src_cfg.sampleRate() << " Hz" << std::endl
        << " target baud rate: " << _baud << std::endl
        << " approx. samples per bit: " << _corrLen;
    Logger::get().log(msg);
    this->setConfig(Config(Config::typeId<uint8_t>(), src_cfg.sampleRate(), src_cfg.bufferSize(), 1));   // :64
  }

protected:
  float _baud;
  size_t _corrLen;
  float _Fmark, _Fspace;
};

/** Drop-in for sdr::ASKDetector<int16_t> (reference src/fsk.hh:69-118). */
template <class Scalar> class ASKDetector;
template <>
class ASKDetector<int16_t> : public detail::DetectorBase {
public:
  explicit ASKDetector(bool invert = false, int device = 0) : detail::DetectorBase("ASKDetector", device), _invert(invert) {}
  virtual void config(const Config &src_cfg) {
    if (!src_cfg.hasType() || !src_cfg.hasSampleRate()) return;
    detail::checkType<int16_t>(src_cfg, "ASKDetector");
    _plan_(SDRHIP_DET_ASK, 0, 0, 0, _invert, src_cfg.bufferSize());
    LogMessage msg(LOG_DEBUG);
    msg << "Config ASKDetector node: " << std::endl
        << " threshold:   " << 0 << std::endl
        << " invert:      " << (_invert ? "yes" : "no") << std::endl
        << " symbol rate: " << src_cfg.sampleRate() << " Hz";
    Logger::get().log(msg);
    this->setConfig(Config(Config::typeId<uint8_t>(), src_cfg.sampleRate(), src_cfg.bufferSize(), 1));   // src/fsk.hh:103
  }

protected:
  bool _invert;
};

// =================================================================================================
// SubSample<complex<int16_t>|complex<float>>
// =================================================================================================
template <class Scalar>
class SubSample : public Sink<Scalar>, public Source {
public:
  explicit SubSample(size_t n, int device = 0) : _n(n), _oFs(0), _device(device) {}
  explicit SubSample(double Fs, int device = 0) : _n(1), _oFs(Fs), _device(device) {}
  virtual ~SubSample() { _buffer.unref(); }
  virtual void config(const Config &src_cfg) {
    if (!src_cfg.hasType() || !src_cfg.hasBufferSize()) return;
    detail::checkType<Scalar>(src_cfg, "SubSample node", "buffer type");
    if (_oFs > 0) _n = size_t(std::max(1.0, src_cfg.sampleRate() / _oFs));
    size_t out_size = src_cfg.bufferSize() / _n;
    if (src_cfg.bufferSize() % _n) out_size += 1;
    detail::configCheck(sdrhip_subsample_create(Device::get(_device), detail::TypeTag<Scalar>::dtype, _n, 1, src_cfg.bufferSize(), _plan.out()),
                        "SubSample");
    _buffer.unref();
    _buffer = Buffer<Scalar>(out_size);
    this->setConfig(Config(src_cfg.type(), src_cfg.sampleRate() / _n, out_size, 1));
  }
  virtual void process(const Buffer<Scalar> &buffer, bool allow_overwrite) {
    if (!_plan) return;
    if (allow_overwrite) _process(buffer, buffer);
    else if (_buffer.isUnused()) _process(buffer, _buffer);
  }

protected:
  void _process(const Buffer<Scalar> &in, const Buffer<Scalar> &out) {
    size_t n = 0;
    if (!detail::processOk(sdrhip_subsample_process(_plan, in.data(), in.size(), 0, out.data(), out.size(), &n), "gpu::SubSample")) return;
    this->send(out.head(n), true);
  }
  size_t _n;
  double _oFs;
  int _device;
  detail::Handle<sdrhip_subsample, sdrhip_subsample_destroy> _plan;
  Buffer<Scalar> _buffer;
};

// =================================================================================================
// FilterNode<float|double>: FFT filter bank (one forward transform's worth of input, several band filters)
// =================================================================================================
namespace detail {
/** The complex<float> / complex<double> entry points of the FFT filter behind one set of names. */
template <class Scalar> struct FftConvApi;
template <> struct FftConvApi<float> {
  static int create(sdrhip_ctx *c, int fft, const float *K, int bands, size_t max_in, sdrhip_fftconv **out) {
    return sdrhip_fftconv_create_bank(c, SDRHIP_FFTCONV_OLA, fft, K, 0, bands, 1, max_in, out); }
  static int setKernel(sdrhip_fftconv *h, int band, const float *K) { return sdrhip_fftconv_set_kernel(h, band, K); }
  static int process(sdrhip_fftconv *h, const float *in, size_t n, float *out) { return sdrhip_fftconv_process(h, in, n, 0, out, 0); }
};
template <> struct FftConvApi<double> {
  static int create(sdrhip_ctx *c, int fft, const double *K, int bands, size_t max_in, sdrhip_fftconv **out) {
    return sdrhip_fftconv_f64_create_bank(c, SDRHIP_FFTCONV_OLA, fft, K, 0, bands, 1, max_in, out); }
  static int setKernel(sdrhip_fftconv *h, int band, const double *K) { return sdrhip_fftconv_f64_set_kernel(h, band, K); }
  static int process(sdrhip_fftconv *h, const double *in, size_t n, double *out) { return sdrhip_fftconv_f64_process(h, in, n, 0, out, 0); }
};
}  // namespace detail

// =================================================================================================
// FilterSink<float|double> / FilterSource<float|double>: the split FFT filter with its spectrum stream in the open
// =================================================================================================
template <class Scalar> class FilterSource;

/** Drop-in for sdr::FilterSink<Scalar>, Scalar = float or double (reference src/filternode.hh:32-99): every buffer of
 * block_size samples becomes one 2 x block_size-point spectrum (zero-padded block, forward DFT, natural order), sent as
 * complex<Scalar>. The config it propagates says bufferSize = block_size, as the reference's does (:76-77), although its
 * buffers hold 2 x block_size points. When every connected sink is connected DIRECT and is a gpu::FilterSource<Scalar> on
 * the same device, the spectrum stays on the device (no copy per block) and the buffer sent is left unfilled; otherwise it
 * is copied into the buffer. */
template <class Scalar>
class FilterSink : public Sink< std::complex<Scalar> >, public Source {
public:
  typedef std::complex<Scalar> CScalar;
  FilterSink(size_t block_size, int device = 0)
    : _block(block_size), _device(device), _out(2 * block_size), _onDevice(false) {}
  virtual ~FilterSink() { _out.unref(); }

  virtual void config(const Config &src_cfg) {
    if ((Config::Type_UNDEFINED == src_cfg.type()) || (0 == src_cfg.sampleRate()) || (0 == src_cfg.bufferSize())) return;
    detail::checkType<CScalar>(src_cfg, "filter-sink");
    if (_block != src_cfg.bufferSize()) {
      ConfigError err;
      err << "Can not configure filter-sink: Invalid buffer size " << src_cfg.bufferSize() << ", expected " << _block;
      throw err;
    }
    if (!_plan) {
      sdrhip_ctx *c = Device::get(_device);
      detail::configCheck(sdrhip_fftsink_create(c, detail::TypeTag<CScalar>::dtype, int(_block), 1, 1, _plan.out()), "gpu::FilterSink");
      _in.alloc(c, _block * sizeof(CScalar), "gpu::FilterSink");
      _spec.alloc(c, 2 * _block * sizeof(CScalar), "gpu::FilterSink");
    }
    setConfig(Config(Config::typeId<CScalar>(), src_cfg.sampleRate(), src_cfg.bufferSize(), src_cfg.numBuffers()));
  }

  virtual void process(const Buffer<CScalar> &buffer, bool) {
    if (!_plan || buffer.size() != _block) return;
    _onDevice = detail::allSinksDirectOn< gpu::FilterSource<Scalar> >(this->_sinks, _device);
    if (!_onDevice) {
      // the repo's drop rule: a buffer still referenced downstream is not overwritten
      if (!_out.isUnused()) return;
      if (!detail::processOk(sdrhip_fftsink_process(_plan, buffer.data(), _block, 0, _out.data(), 0), "gpu::FilterSink")) return;
      send(_out);
      return;
    }
    sdrhip_ctx *c = Device::get(_device);
    if (!detail::processOk(sdrhip_memcpy_h2d(c, _in.get(), buffer.data(), _block * sizeof(CScalar)), "gpu::FilterSink") ||
        !detail::processOk(sdrhip_fftsink_process_dev(_plan, _in.get(), _block, 0, _spec.get(), 0), "gpu::FilterSink")) return;
    const detail::HandoffScope handoff(_out.data(), _spec.get(), _device);
    send(_out);
  }

  /** true: the last block's spectrum went to the sources on the device (no host copy). */
  bool lastBlockOnDevice() const { return _onDevice; }
  size_t blockSize() const { return _block; }
  int device() const { return _device; }

protected:
  size_t _block;
  int _device;
  detail::Handle<sdrhip_fftsink, sdrhip_fftsink_destroy> _plan;
  detail::DeviceMem _in, _spec;
  Buffer<CScalar> _out;
  bool _onDevice;
};

/** Drop-in for sdr::FilterSource<Scalar>, Scalar = float or double (reference src/filternode.hh:103-227): a Sink of the
 * 2 x block_size-point spectra FilterSink sends, a Source of block_size filtered samples. Per block: spectrum x kernel,
 * inverse DFT, / 2N, and the upper half of the last block's result added (overlap-add, the tail carried on the device).
 * The kernel is sinc_flt_kernel + _updateFilter's spectrum (:18-28,186-203), made at config and by setFreq, which applies it
 * from the next block and keeps the tail: the block after it is the OLD kernel's tail plus the NEW kernel's head, exactly
 * as the reference's. A block whose output buffer is still referenced downstream is dropped; the kernel still runs, so
 * that the tail stays aligned with the input. */
template <class Scalar>
class FilterSource : public Sink< std::complex<Scalar> >, public Source {
public:
  typedef std::complex<Scalar> CScalar;
  FilterSource(size_t block_size, double fmin, double fmax, int device = 0)
    : FilterSource(Inert(), block_size, fmin, fmax, device) { _inert = false; }
  virtual ~FilterSource() { _buffer.unref(); }

  /** FilterSource::setFreq (:128-130): the kernel is recomputed (once configured) and applies from the next block. */
  virtual void setFreq(double fmin, double fmax) {
    _fmin = fmin; _fmax = fmax;
    if (_plan) detail::configCheck(sdrhip_fftsource_set_kernel(_plan, _kernel().data()), "FilterSource");
  }
  virtual double fmin() const { return _fmin; }
  virtual double fmax() const { return _fmax; }
  /** true: the last block's spectrum came from a gpu::FilterSink on the device (no upload). */
  bool lastBlockOnDevice() const { return _onDevice; }
  int device() const { return _device; }

  virtual void config(const Config &src_cfg) {
    if (_inert) return;
    if ((0 == src_cfg.sampleRate()) || (0 == src_cfg.bufferSize())) return;
    if (_block != src_cfg.bufferSize()) {
      ConfigError err;
      err << "Can not configure FilterSource, block-size (=" << _block << ") != buffer-size (=" << src_cfg.bufferSize() << ")!";
      throw err;
    }
    _Fs = src_cfg.sampleRate();
    const std::vector<Scalar> K = _kernel();
    if (!_plan) {
      sdrhip_ctx *c = Device::get(_device);
      detail::configCheck(sdrhip_fftsource_create(c, detail::TypeTag<CScalar>::dtype, int(_block), K.data(), 1, 1, _plan.out()),
                          "FilterSource");
      _spec.alloc(c, 2 * _block * sizeof(CScalar), "FilterSource");
      _outDev.alloc(c, _block * sizeof(CScalar), "FilterSource");
      _buffer = Buffer<CScalar>(_block);
      _scratch.resize(_block);
    } else {
      detail::configCheck(sdrhip_fftsource_set_kernel(_plan, K.data()), "FilterSource");
    }
    Source::setConfig(Config(Config::typeId<CScalar>(), src_cfg.sampleRate(), _block, src_cfg.numBuffers()));
  }

  virtual void process(const Buffer<CScalar> &buffer, bool) {
    if (_inert || !_plan || buffer.size() < 2 * _block) return;
    sdrhip_ctx *c = Device::get(_device);
    const bool keep = _buffer.isUnused();
    const void *handed = detail::handoffFor(buffer.data(), _device);
    _onDevice = handed != 0;
    const void *spec = _onDevice ? handed : _spec.get();
    if (!_onDevice && !detail::processOk(sdrhip_memcpy_h2d(c, _spec.get(), buffer.data(), 2 * _block * sizeof(CScalar)), "FilterSource"))
      return;
    if (!detail::processOk(sdrhip_fftsource_process_dev(_plan, spec, 1, 0, _outDev.get(), 0), "FilterSource")) return;
    CScalar *dst = keep ? reinterpret_cast<CScalar *>(_buffer.data()) : _scratch.data();
    if (!detail::processOk(sdrhip_memcpy_d2h(c, dst, _outDev.get(), _block * sizeof(CScalar)), "FilterSource") || !keep) return;
    send(_buffer);
  }

protected:
  /** Band of gpu::FilterNode: no device state, its sink side does nothing (the bank runs it). */
  struct Inert {};
  FilterSource(Inert, size_t block_size, double fmin, double fmax, int device)
    : _block(block_size), _fmin(fmin), _fmax(fmax), _device(device), _Fs(0), _onDevice(false), _inert(true) {}
  std::vector<Scalar> _kernel() const { return detail::fftFilterSpectrum<Scalar>(_block, _fmin, _fmax, _Fs); }
  size_t _block;
  double _fmin, _fmax;
  int _device;
  double _Fs;
  detail::Handle<sdrhip_fftsource, sdrhip_fftsource_destroy> _plan;
  detail::DeviceMem _spec, _outDev;
  bool _onDevice, _inert;
  Buffer<CScalar> _buffer;
  std::vector<CScalar> _scratch;
};

/** Drop-in for sdr::FilterNode<Scalar>, Scalar = float or double (reference src/filternode.hh:230-284), ANY block size
 * (:235: `FilterNode(size_t block_size=1024)`; FFTW plans any 2 x block_size): one launch per buffer where the transform
 * fits a workgroup's LDS and is made of the factors 2 ... 13, passes over device memory around a four-step / chirp
 * plan otherwise (csrc/fftany.hpp). */
template <class Scalar>
class FilterNode {
public:
  typedef std::complex<Scalar> CScalar;
  /** One band of the bank: a gpu::FilterSource<Scalar> (src/filternode.hh:105-227) whose sink side is inert — the bank
   * runs it — so that `gpu::FilterSource<Scalar> *s = bank.addFilter(a, b)` works as with the reference's FilterNode. */
  class Band : public gpu::FilterSource<Scalar> {
  public:
    Band(FilterNode *p, size_t index, double fmin, double fmax)
      : gpu::FilterSource<Scalar>(typename gpu::FilterSource<Scalar>::Inert(), p->_block, fmin, fmax, p->_device), _p(p), _index(index) {}
    /** FilterSource::setFreq (:132-139): only this band's kernel is recomputed; the overlap history goes on. */
    virtual void setFreq(double fmin, double fmax) {
      if (fmax < fmin) std::swap(fmin, fmax);
      this->_fmin = fmin; this->_fmax = fmax;
      _p->_bandChanged(_index);
    }

  protected:
    friend class FilterNode;
    FilterNode *_p;
    size_t _index;
  };

  explicit FilterNode(size_t block_size = 1024, int device = 0) : _block(block_size), _device(device), _sink(this) {}
  virtual ~FilterNode() {
    for (size_t b = 0; b < _bands.size(); b++) delete _bands[b];
  }

  /** The input of the bank. Unlike the reference (whose BufferNode crashes: SURVEY fact 7) any buffer size is accepted. */
  Sink<CScalar> *sink() { return &_sink; }
  /** Adds a band [fmin, fmax]; the returned Source emits the filtered stream. Adding a band to a configured bank makes
   * a new device plan (the bands' overlap history restarts). */
  Band *addFilter(double fmin, double fmax) {
    if (fmax < fmin) std::swap(fmin, fmax);
    _bands.push_back(new Band(this, _bands.size(), fmin, fmax));
    if (_cfg.hasSampleRate()) _configure(_cfg);
    return _bands.back();
  }

protected:
  std::vector<Scalar> _kernelOf(const Band *b) const { return detail::fftFilterSpectrum<Scalar>(_block, b->_fmin, b->_fmax, _cfg.sampleRate()); }
  /** ONE device plan for all bands: one upload and one forward FFT per input block feed every band
   * (FilterSink -> FilterSource fan-out, src/filternode.hh:81-88,257-270). */
  void _configure(const Config &cfg) {
    _cfg = cfg;
    _plan.reset();
    if (_bands.empty()) return;
    std::vector<Scalar> K;
    for (size_t b = 0; b < _bands.size(); b++) { const std::vector<Scalar> k = _kernelOf(_bands[b]); K.insert(K.end(), k.begin(), k.end()); }
    detail::configCheck(detail::FftConvApi<Scalar>::create(Device::get(_device), int(2 * _block), K.data(), int(_bands.size()),
                                                           cfg.bufferSize(), _plan.out()), "FFT filter");
    _stage.resize(2 * cfg.bufferSize() * _bands.size());
    for (size_t b = 0; b < _bands.size(); b++) {
      _bands[b]->_buffer.unref();
      _bands[b]->_buffer = Buffer<CScalar>(cfg.bufferSize());
      _bands[b]->setConfig(Config(Config::typeId<CScalar>(), cfg.sampleRate(), cfg.bufferSize(), 1));
    }
  }
  void _bandChanged(size_t index) {
    if (!_plan) return;
    detail::configCheck(detail::FftConvApi<Scalar>::setKernel(_plan, int(index), _kernelOf(_bands[index]).data()), "FFT filter");
  }
  void _run(const Buffer<CScalar> &in) {
    if (!_plan || in.size() * 2 * _bands.size() > _stage.size()) return;
    // a band whose output buffer is still referenced downstream drops this block (src/baseband.hh:141-150 rule); the
    // bank still runs, so that every band's overlap history stays aligned with the input
    if (!detail::processOk(detail::FftConvApi<Scalar>::process(_plan, reinterpret_cast<const Scalar *>(in.data()), in.size(), _stage.data()),
                           "gpu::FilterNode")) return;
    for (size_t b = 0; b < _bands.size(); b++) {
      Band *bd = _bands[b];
      if (!bd->_buffer.isUnused()) continue;
      memcpy(bd->_buffer.data(), _stage.data() + b * 2 * in.size(), in.size() * sizeof(CScalar));
      bd->send(bd->_buffer.head(in.size()), false);
    }
  }

  class In : public Sink<CScalar> {
  public:
    explicit In(FilterNode *p) : _p(p) {}
    virtual void config(const Config &src_cfg) {
      if (Config::Type_UNDEFINED == src_cfg.type() || 0 == src_cfg.sampleRate() || 0 == src_cfg.bufferSize()) return;
      detail::checkType<CScalar>(src_cfg, "filter-sink");
      _p->_configure(src_cfg);
    }
    virtual void process(const Buffer<CScalar> &buffer, bool) { _p->_run(buffer); }
    FilterNode *_p;
  };
  friend class Band;
  size_t _block;
  int _device;
  Config _cfg;
  detail::Handle<sdrhip_fftconv, sdrhip_fftconv_destroy> _plan;
  In _sink;
  std::vector<Band *> _bands;
  std::vector<Scalar> _stage;
};

// =================================================================================================
// ChannelBank<int16_t>: C independent IQBaseBand<int16_t>(+demod) channels, one batched launch per device
// =================================================================================================
template <class Scalar> class ChannelBank;

/** Many independent channels behind one port per channel — sink(c) / source(c), the reference's own pattern for
 * multi-input nodes (Combine::sink(i), src/combine.hh:66-150). The channels are split into contiguous blocks over
 * the given devices (one rank each, sdrhip_comm_*): every device filters its block in one batched launch, no data
 * path collective; the demodulated rows are gathered on rank 0's device (RCCL over xGMI when the devices differ)
 * and leave in one device-to-host copy — BASELINE config 5's shape, driven from C++ in one process. The staging
 * buffers are pinned (registered), so each device's copies are plain DMA on its own stream and run beside the
 * other devices' kernels. */
template <>
class ChannelBank<int16_t> {
public:
  class Out : public Source {
  public:
    void configure(const Config &c) { this->setConfig(c); }
    void emit(const RawBuffer &b, bool aw) { this->send(b, aw); }
    /** true while some sink is connected (a bank copies a row to the host only for one that has a receiver) */
    bool connected() const { return !this->_sinks.empty(); }
  };

  /** All channels share the band-select parameters (taps / LUT are read-only data, designed once on the host). */
  ChannelBank(size_t channels, double Fc, double Ff, double width, size_t order, size_t sub_sample, int epilogue = SDRHIP_EPI_NONE,
              int device = 0)
    : ChannelBank(channels, Fc, Ff, width, order, sub_sample, epilogue, std::vector<int>(1, device)) {}
  /** The same bank over several devices: rank r (device devices[r]) owns the r-th contiguous block of channels. */
  ChannelBank(size_t channels, double Fc, double Ff, double width, size_t order, size_t sub_sample, int epilogue,
              const std::vector<int> &devices)
    : _C(channels), _Fc(Fc), _Ff(Ff), _width(width), _order(std::max(size_t(1), order)), _D(sub_sample), _epilogue(epilogue),
      _devices(devices.empty() ? std::vector<int>(1, 0) : devices), _bs(0), _have(0), _ins(channels, In(this)),
      _outs(channels), _pending(channels, false) {
    for (size_t c = 0; c < _C; c++) _ins[c]._index = c;
  }
  virtual ~ChannelBank() {
    _release();
    _stageOut.unref();
    _stageIn.unref();
  }
  Sink<cs16> *sink(size_t c) { return &_ins[c]; }
  Source *source(size_t c) { return &_outs[c]; }
  size_t channels() const { return _C; }
  size_t ranks() const { return _devices.size(); }
  /** "rccl" or "same-device copies" once configured (sdrhip_comm_transport). */
  const char *transport() const { const char *n = ""; if (_comm) sdrhip_comm_transport(_comm, &n); return n; }

protected:
  class In : public Sink<cs16> {
  public:
    explicit In(ChannelBank *p) : _p(p), _index(0) {}
    virtual void config(const Config &cfg) { _p->_config(cfg); }
    virtual void process(const Buffer<cs16> &b, bool) { _p->_deliver(_index, b); }
    ChannelBank *_p;
    size_t _index;
  };
  struct Rank {
    sdrhip_ctx *ctx; detail::Handle<sdrhip_iqbb_i16, sdrhip_iqbb_i16_destroy> plan; size_t c0, c1; detail::DeviceMem din, dout;
    Rank() : ctx(0), c0(0), c1(0) {}
  };

  /** In this order: the ranks' contexts belong to the comm, which therefore goes last, after all work on them has ended. */
  void _release() {
    if (_comm) sdrhip_comm_synchronize(_comm);
    for (size_t r = 0; r < _ranks.size(); r++) { _ranks[r].plan.reset(); _ranks[r].din.reset(); _ranks[r].dout.reset(); }
    _gather.reset();
    _ranks.clear();
    _pinIn.reset();
    _pinOut.reset();
    _comm.reset();
  }

  void _config(const Config &cfg) {
    if (!cfg.hasType() || !cfg.hasSampleRate() || !cfg.hasBufferSize()) return;
    detail::checkType<cs16>(cfg, "ChannelBank");
    if (_comm && cfg == _cfg) return;   // every channel's source pushes the same Config
    _cfg = cfg;
    _bs = cfg.bufferSize();
    const int32_t Fs = int32_t(cfg.sampleRate());
    const std::vector<int32_t> taps = detail::iqbbTaps(_Ff, _width, Fs, _order), lut = detail::freqShiftLut();
    _release();
    _stageIn.unref(); _stageOut.unref();
    _outStride = _bs / _D + 2;
    _stageIn = Buffer<cs16>(_C * _bs);
    _stageOut = Buffer<cs16>(_C * _outStride);
    _pinIn.reset(_stageIn.data(), _C * _bs * sizeof(cs16), "ChannelBank");
    _pinOut.reset(_stageOut.data(), _C * _outStride * sizeof(cs16), "ChannelBank");
    const size_t R = std::min(_devices.size(), _C);
    detail::configCheck(sdrhip_comm_create(_devices.data(), int(R), _comm.out()), "ChannelBank");
    _ranks.resize(R);
    for (size_t r = 0; r < R; r++) {   // contiguous blocks, sizes differ by at most one
      Rank &k = _ranks[r];
      k.c0 = r * (_C / R) + std::min(r, _C % R);
      k.c1 = k.c0 + _C / R + (r < _C % R ? 1 : 0);
      detail::configCheck(sdrhip_comm_ctx(_comm, int(r), &k.ctx), "ChannelBank");
      detail::configCheck(sdrhip_iqbb_i16_create(k.ctx, taps.data(), int(_order), lut.data(), design::freqShiftIncrement(_Fc, double(Fs)),
                                                 0 > _Fc, int(_D), int(k.c1 - k.c0), _bs, _epilogue, k.plan.out()), "ChannelBank");
      k.din.alloc(k.ctx, (k.c1 - k.c0) * _bs * sizeof(cs16), "ChannelBank");
      k.dout.alloc(k.ctx, (k.c1 - k.c0) * _outStride * sizeof(cs16), "ChannelBank");
    }
    if (R > 1) _gather.alloc(_ranks[0].ctx, _C * _outStride * sizeof(cs16), "ChannelBank");
    std::fill(_pending.begin(), _pending.end(), false);
    _chunkHave.assign((_C + kChunk - 1) / kChunk, 0);
    _copyOk = true;
    _have = 0;
    for (size_t c = 0; c < _C; c++) _outs[c].configure(detail::bankOutConfig(_epilogue, Fs, _D, _outStride));
  }

  /** Collects one buffer per channel (all of the same length: buffer boundaries are part of the
   * numerical contract), then launches once per device for the whole bank. */
  void _deliver(size_t c, const Buffer<cs16> &b) {
    if (!_comm || b.size() > _bs) return;
    if (_have == 0) { _len = b.size(); _copyOk = true; }
    if (_pending[c] || b.size() != _len) {
      LogMessage msg(LOG_WARNING);
      msg << "gpu::ChannelBank: channel " << c << " delivered out of step; buffer dropped";
      Logger::get().log(msg);
      return;
    }
    memcpy(_stageIn.data() + c * _bs * sizeof(cs16), b.data(), b.size() * sizeof(cs16));
    _pending[c] = true;
    // The round's input travels while the round is still being delivered: the channels come one buffer at a time from the
    // caller's thread (a 256 KB memcpy each into the pinned staging area: 10 ms for 1024 channels on one core), so every
    // completed chunk of kChunk channels starts its H2D copy at once and the copies hide behind the memcpys of the chunks
    // that follow (measured through examples/bench_graph.cc: profiles/r18_host_path.txt)
    const size_t k = c / kChunk;
    if (++_chunkHave[k] == std::min<size_t>(kChunk, _C - k * kChunk)) _copyChunk(k);
    if (++_have < _C) return;
    _have = 0;
    std::fill(_pending.begin(), _pending.end(), false);
    std::fill(_chunkHave.begin(), _chunkHave.end(), 0);
    // the per-channel outputs are views of _stageOut: while a consumer (e.g. a queued edge) still holds one of the
    // last round, this round is dropped, as every node drops its input while its output buffer is in use
    // (src/baseband.hh:141-150)
    if (!_stageOut.isUnused()) {
      LogMessage msg(LOG_WARNING);
      msg << "gpu::ChannelBank: output of the last round still in use downstream; round dropped";
      Logger::get().log(msg);
      return;
    }
    size_t n = 0;
    const size_t per = detail::fusedPer<cs16>(_epilogue);   // int16 elements fit twice into a cs16 row
    const size_t R = _ranks.size(), rowB = _outStride * sizeof(cs16);
    std::vector<const void *> send(R); std::vector<size_t> bytes(R);
    bool ok = _copyOk;
    for (size_t r = 0; r < R && ok; r++) {   // every rank: its batched launch behind its chunks' H2D copies (same stream), all asynchronous
      Rank &k = _ranks[r];
      ok = detail::processOk(sdrhip_iqbb_i16_process_dev(k.plan, k.din.as<int16_t>(), _len, _bs, k.dout.get(),
                                                         _outStride * per, &n), "gpu::ChannelBank");
      send[r] = k.dout.get(); bytes[r] = (k.c1 - k.c0) * rowB;
    }
    if (ok && R > 1)   // rows gathered on rank 0's device in channel order (RCCL over xGMI), then one copy to the host
      ok = detail::processOk(sdrhip_comm_gather(_comm, send.data(), bytes.data(), _gather.get(), 0), "gpu::ChannelBank") &&
           detail::processOk(sdrhip_memcpy_d2h_async(_ranks[0].ctx, _stageOut.data(), _gather.get(), _C * rowB), "gpu::ChannelBank");
    else if (ok)
      ok = detail::processOk(sdrhip_memcpy_d2h_async(_ranks[0].ctx, _stageOut.data(), _ranks[0].dout.get(), _C * rowB), "gpu::ChannelBank");
    if (!detail::processOk(sdrhip_comm_synchronize(_comm), "gpu::ChannelBank") || !ok) return;
    for (size_t ch = 0; ch < _C; ch++) detail::sendDemodulated(_outs[ch], _epilogue, _stageOut, ch * _outStride, n, false);
  }

  /** H2D copy of the channels [k * kChunk, (k + 1) * kChunk) of the round being collected: each rank's part on that rank's stream. */
  void _copyChunk(size_t k) {
    const size_t a = k * kChunk, b = std::min<size_t>(_C, a + kChunk);
    for (size_t r = 0; r < _ranks.size(); r++) {
      Rank &rk = _ranks[r];
      const size_t lo = std::max(a, rk.c0), hi = std::min(b, rk.c1);
      if (lo >= hi) continue;
      if (!detail::processOk(sdrhip_memcpy_h2d_async(rk.ctx, rk.din.as<char>() + (lo - rk.c0) * _bs * sizeof(cs16),
                                                     _stageIn.data() + lo * _bs * sizeof(cs16), (hi - lo) * _bs * sizeof(cs16)), "gpu::ChannelBank"))
        _copyOk = false;
    }
  }

  enum { kChunk = 32 };   // channels per H2D chunk (an enumerator: no out-of-class definition needed when bound to a reference)
  std::vector<size_t> _chunkHave;
  bool _copyOk = true;
  size_t _C;
  double _Fc, _Ff, _width;
  size_t _order, _D;
  int _epilogue;
  std::vector<int> _devices;
  detail::Handle<sdrhip_comm, sdrhip_comm_destroy> _comm;
  std::vector<Rank> _ranks;
  detail::DeviceMem _gather;
  detail::Pinned _pinIn, _pinOut;   // the registrations of _stageIn and _stageOut
  Config _cfg;
  size_t _bs, _have, _len, _outStride;
  std::vector<In> _ins;
  std::vector<Out> _outs;
  std::vector<bool> _pending;
  Buffer<cs16> _stageIn, _stageOut;
};

// =================================================================================================
// TunerBank<int16_t>: ONE wideband input, C IQBaseBand<int16_t>(+demod) channels each with its own tune and filter
// =================================================================================================
template <class Scalar> class TunerBank;

namespace detail {
/** What the two kinds of bank differ in: the sample type, how the node keeps its frequencies and derives its output rate
 * (IQBaseBand: int32 members, truncated, and the integer quotient, src/baseband.hh:266-272; the real-input BaseBand: doubles
 * and the double quotient, :357-395,520-526), the tap design and the create calls. */
struct ComplexBank {
  typedef cs16 In;
  typedef int32_t Freq;
  static const char *name() { return "TunerBank"; }
  static const char *gname() { return "gpu::TunerBank"; }
  static double outRate(Freq Fs, size_t D) { return double(size_t(Fs) / D); }
  static void taps(double Ff, double width, double Fs, size_t order, int32_t *dst) { design::iqbbTaps(Ff, width, Fs, order, dst); }
  static int create(sdrhip_ctx *ctx, const int32_t *taps, int order, const int32_t *lut, const uint32_t *inc, const int *neg, const int *modes,
                    int D, int C, size_t bs, int epilogue, sdrhip_tuner_i16 **out) {
    return modes ? sdrhip_tunermodes_i16_create(ctx, taps, order, lut, inc, neg, modes, D, C, bs, out)
                 : sdrhip_tuner_i16_create(ctx, taps, order, lut, inc, neg, D, C, bs, epilogue, out);
  }
};
struct RealBank {
  typedef int16_t In;
  typedef double Freq;
  static const char *name() { return "RealTunerBank"; }
  static const char *gname() { return "gpu::RealTunerBank"; }
  static double outRate(Freq Fs, size_t D) { return Fs / double(D); }
  static void taps(double Ff, double width, double Fs, size_t order, int32_t *dst) { design::bbTaps(Ff, width, Fs, order, dst); }
  static int create(sdrhip_ctx *ctx, const int32_t *taps, int order, const int32_t *lut, const uint32_t *inc, const int *neg, const int *modes,
                    int D, int C, size_t bs, int epilogue, sdrhip_tuner_i16 **out) {
    return modes ? sdrhip_tunermodes_bb_i16_create(ctx, taps, order, lut, inc, neg, modes, D, C, bs, out)
                 : sdrhip_tunerbb_i16_create(ctx, taps, order, lut, inc, neg, D, C, bs, epilogue, out);
  }
};

/** The node both kinds of bank are (TunerBank<int16_t> and RealTunerBank<int16_t> below say what it does). */
template <class K>
class TunerBank16 : public Sink<typename K::In> {
public:
  typedef typename K::In In;
  typedef typename K::Freq Freq;
  typedef ChannelBank<int16_t>::Out Out;
  /** The constructor's `epilogue` of a bank with a demodulator per channel. */
  enum { PerChannel = -1 };

  TunerBank16(size_t order, size_t sub_sample, int epilogue, int device)
    : _order(std::max(size_t(1), order)), _D(std::max(size_t(1), sub_sample)), _epilogue(epilogue), _device(device), _ctx(0),
      _bs(0), _outStride(0), _Fs(0) {}
  virtual ~TunerBank16() {
    _release();
    for (size_t c = 0; c < _outs.size(); c++) delete _outs[c];
  }

  /** A new channel; returns its index. Before or after config(). Its demodulator is the bank's; FMDemod in a bank with one per
   * channel. */
  size_t addChannel(double Fc, double Ff, double width) { return addChannel(Fc, Ff, width, perChannel() ? int(SDRHIP_EPI_FM) : _epilogue); }
  /** ... with the demodulator `mode`: SDRHIP_EPI_FM | _AM | _USB in a bank with one per channel; in any other bank a mode that
   * is not the bank's throws ConfigError. */
  size_t addChannel(double Fc, double Ff, double width, int mode) {
    _checkMode(mode);
    _tunes.push_back(Tune(Fc, Ff, width));
    _modes.push_back(mode);
    _outs.push_back(new Out());
    if (_plan) _rebuild();
    return _tunes.size() - 1;
  }
  size_t channels() const { return _tunes.size(); }
  bool perChannel() const { return _epilogue == PerChannel; }
  /** The demodulator of channel c (the bank's, where it has one for all). */
  int mode(size_t c) const { return _modes[c]; }
  /** A new demodulator node behind channel c's baseband. Before config() the mode is only recorded; afterwards the running plan
   * changes between two buffers (sdrhip_tunermodes_i16_set_mode): the baseband continues, a new FMDemod starts from angle 0, no other
   * channel is touched. In a bank with one demodulator for all, a mode that is not the bank's throws ConfigError. */
  void setMode(size_t c, int mode) {
    _checkMode(mode);
    if (!perChannel()) return;
    if (_plan) detail::configCheck(sdrhip_tunermodes_i16_set_mode(_plan, int(c), mode), K::name());
    _modes[c] = mode;
  }
  Source *source(size_t c) { return _outs[c]; }

  double centerFrequency(size_t c) const { return _tunes[c].Fc; }
  double filterFrequency(size_t c) const { return _tunes[c].Ff; }
  double filterWidth(size_t c) const { return _tunes[c].width; }
  /** The reference setters' effects (src/baseband.hh:82-104) on channel c alone. */
  void setCenterFrequency(size_t c, double Fc) {
    Tune &t = _tunes[c];
    t.Fc = Freq(Fc); t.shift = t.Fc;   // (IQBaseBand: truncated before setFrequencyShift, src/baseband.hh:85)
    if (_plan) detail::configCheck(sdrhip_tuner_i16_set_shift(_plan, int(c), design::freqShiftIncrement(t.shift, double(_Fs)), 0 > t.shift), K::name());
  }
  void setFilterFrequency(size_t c, double Ff) { _tunes[c].Ff = Freq(Ff); _retap(c); }
  void setFilterWidth(size_t c, double width) { _tunes[c].width = Freq(width); _retap(c); }

  virtual void config(const Config &cfg) {
    if (!cfg.hasType() || !cfg.hasSampleRate() || !cfg.hasBufferSize()) return;
    detail::checkType<In>(cfg, K::name());
    _bs = cfg.bufferSize();
    _Fs = Freq(cfg.sampleRate());
    _rebuild();
  }

  virtual void process(const Buffer<In> &b, bool) {
    if (!_plan || b.size() > _bs) return;
    // the per-channel outputs are views of _stageOut: while a consumer still holds one of the last round, this round is
    // dropped, as every node drops its input while its output buffer is in use (src/baseband.hh:141-150)
    if (!_stageOut.isUnused()) {
      LogMessage msg(LOG_WARNING);
      msg << K::gname() << ": output of the last round still in use downstream; buffer dropped";
      Logger::get().log(msg);
      return;
    }
    const size_t C = _tunes.size(), per = detail::fusedPer<cs16>(_epilogue);   // int16 elements fit twice into a cs16 row
    size_t n = 0;
    if (b.size() == 0) return;
    if (!detail::processOk(sdrhip_memcpy_h2d_async(_ctx, _din.get(), b.data(), b.size() * sizeof(In)), K::gname()) ||
        !detail::processOk(sdrhip_tuner_i16_process_dev(_plan, _din.get(), b.size(), _dout.get(), _outStride * per, &n), K::gname()) ||
        !detail::processOk(sdrhip_memcpy_d2h_async(_ctx, _stageOut.data(), _dout.get(), C * _outStride * sizeof(cs16)), K::gname()) ||
        !detail::processOk(sdrhip_ctx_synchronize(_ctx), K::gname()))
      return;
    for (size_t ch = 0; ch < C; ch++) detail::sendDemodulated(*_outs[ch], _modes[ch], _stageOut, ch * _outStride, n, false);
  }

protected:
  // as the reference node keeps them (src/baseband.hh:266-272): int32 members, truncated; only the constructor's frequency
  // shift is the untruncated double (gpu::IQBaseBand: _shift)
  struct Tune {
    Freq Fc, Ff, width;
    double shift;
    Tune(double fc, double ff, double w) : Fc(Freq(fc)), Ff(Freq(ff)), width(Freq(w)), shift(fc) {}
  };

  void _checkMode(int mode) const {
    if (perChannel() ? (mode == SDRHIP_EPI_FM || mode == SDRHIP_EPI_AM || mode == SDRHIP_EPI_USB) : mode == _epilogue) return;
    ConfigError err;
    if (perChannel()) err << K::name() << ": mode " << mode << " is none of SDRHIP_EPI_FM, SDRHIP_EPI_AM, SDRHIP_EPI_USB";
    else err << K::name() << ": mode " << mode << " in a bank whose channels all have the demodulator " << _epilogue;
    throw err;
  }

  void _retap(size_t c) {
    if (!_plan) return;
    std::vector<int32_t> taps(2 * _order);
    K::taps(_tunes[c].Ff, _tunes[c].width, _Fs, _order, taps.data());
    detail::configCheck(sdrhip_tuner_i16_set_taps(_plan, int(c), taps.data()), K::name());
  }

  /** In this order: the device is idle before anything it may still use goes. (Virtual, as _rebuild: gpu::ReceiverBank
   * builds its later stages around this bank's plan.) */
  virtual void _release() {
    if (_ctx) sdrhip_ctx_synchronize(_ctx);
    _plan.reset();
    _din.reset();
    _dout.reset();
    _pinOut.reset();
    _stageOut.unref();
  }

  virtual void _rebuild() {
    _release();
    const size_t C = _tunes.size();
    if (C == 0 || _bs == 0) return;
    _ctx = Device::get(_device);
    std::vector<int32_t> taps(C * 2 * _order);
    const std::vector<int32_t> lut = detail::freqShiftLut();
    std::vector<uint32_t> inc(C);
    std::vector<int> neg(C);
    for (size_t c = 0; c < C; c++) {
      K::taps(_tunes[c].Ff, _tunes[c].width, _Fs, _order, taps.data() + c * 2 * _order);
      inc[c] = design::freqShiftIncrement(_tunes[c].shift, double(_Fs));
      neg[c] = 0 > _tunes[c].shift;
    }
    _outStride = (_bs + _D - 1) / _D + 1;
    detail::configCheck(K::create(_ctx, taps.data(), int(_order), lut.data(), inc.data(), neg.data(), perChannel() ? _modes.data() : 0,
                                  int(_D), int(C), _bs, _epilogue, _plan.out()), K::name());
    _din.alloc(_ctx, _bs * sizeof(In), K::name());
    _dout.alloc(_ctx, C * _outStride * sizeof(cs16), K::name());
    _stageOut = Buffer<cs16>(C * _outStride);
    _pinOut.reset(_stageOut.data(), C * _outStride * sizeof(cs16), K::name());
    for (size_t c = 0; c < C; c++) _outs[c]->configure(Config(detail::fusedType<cs16>(_epilogue), K::outRate(_Fs, _D), _outStride, 1));
  }

  size_t _order, _D;
  int _epilogue, _device;
  sdrhip_ctx *_ctx;
  detail::Handle<sdrhip_tuner_i16, sdrhip_tuner_i16_destroy> _plan;
  detail::DeviceMem _din, _dout;
  detail::Pinned _pinOut;   // the registration of _stageOut
  size_t _bs, _outStride;
  Freq _Fs;
  std::vector<Tune> _tunes;
  std::vector<int> _modes;   // per channel: its demodulator (the bank's epilogue, where it has one for all)
  std::vector<Out *> _outs;
  Buffer<cs16> _stageOut;
};
}  // namespace detail

/** Several IQBaseBand<int16_t> nodes connected to one source, as one node: a Sink<cs16> with one Source per channel
 * (source(c), the ChannelBank::Out pattern). Every channel has its own centre frequency, filter frequency and width;
 * order, sub-sampling and the fused demodulator are the bank's. Per buffer: one H2D copy, one launch for all channels
 * (sdrhip_tuner_i16_*), one D2H copy of all rows into a pinned staging buffer, then one send per channel, in channel
 * order, as views of it. addChannel() after config() rebuilds the device plan: every channel restarts as a freshly
 * configured node (FIR history, decimator and LUT phases at zero).
 * With epilogue = TunerBank::PerChannel every channel has a demodulator of its own (SDRHIP_EPI_FM | _AM | _USB: the modes of
 * the reference's receiver, examples/sdr_rec.cc:44-110, on one antenna), still in one launch; setMode() replaces the
 * demodulator node behind ONE channel's baseband, which goes on as it is (sdrhip_tunermodes_i16_set_mode). Every output's Config
 * is int16_t at the decimated rate, whatever the modes are. */
template <>
class TunerBank<int16_t> : public detail::TunerBank16<detail::ComplexBank> {
public:
  TunerBank(size_t order, size_t sub_sample, int epilogue = SDRHIP_EPI_NONE, int device = 0)
    : detail::TunerBank16<detail::ComplexBank>(order, sub_sample, epilogue, device) {}
};

template <class Scalar> class RealTunerBank;
/** The bank for a real-sampled antenna (a direct-sampling HF receiver): several BaseBand<int16_t> nodes connected to one source
 * of real int16 samples, as one node — a Sink<int16_t> with one Source per channel, everything else as TunerBank<int16_t>:
 * the same constructor forms (RealTunerBank::PerChannel included), addChannel, setMode and the per-channel setters, one launch
 * per buffer (sdrhip_tunerbb_i16_create / sdrhip_tunermodes_bb_i16_create). As the reference's real-input node it keeps
 * its frequencies and the sample rate as doubles (src/baseband.hh:520-526), designs Q16 taps and sends at Fs / sub_sample. */
template <>
class RealTunerBank<int16_t> : public detail::TunerBank16<detail::RealBank> {
public:
  RealTunerBank(size_t order, size_t sub_sample, int epilogue = SDRHIP_EPI_NONE, int device = 0)
    : detail::TunerBank16<detail::RealBank>(order, sub_sample, epilogue, device) {}
};

// =================================================================================================
// FFT::exec / FFTPlan<float|double> on host buffers (reference src/fftplan.hh:14-36, src/fftplan_fftw3.hh:12-142)
// =================================================================================================
/** The reference's FFT module: the same Direction enum, exec<Scalar>(in, out, dir) and exec<Scalar>(inplace, dir). */
template <class Scalar> class FFTPlan;

class FFT {
public:
  typedef enum { FORWARD, BACKWARD } Direction;
  template <class Scalar>
  static void exec(const Buffer< std::complex<Scalar> > &in, const Buffer< std::complex<Scalar> > &out, FFT::Direction dir, int device = 0) {
    FFTPlan<Scalar> plan(in, out, dir, device); plan();
  }
  template <class Scalar>
  static void exec(const Buffer< std::complex<Scalar> > &inplace, FFT::Direction dir, int device = 0) {
    FFTPlan<Scalar> plan(inplace, dir, device); plan();
  }
};

/** FFTPlan<float> and FFTPlan<double>: same constructors and error texts as the FFTW-backed reference classes; the
 * transform is the library's own (unnormalised either way, like FFTW), for ANY size. As in the reference the plan is made
 * ONCE, in the constructor (src/fftplan_fftw3.hh:34-36,52-54: fftw_plan_dft_1d) — a size the device cannot plan is a
 * ConfigError there — and operator() only executes it (:59); the destructor frees it (:64). */
template <class Scalar>
class FFTPlan {
public:
  FFTPlan(const Buffer< std::complex<Scalar> > &in, const Buffer< std::complex<Scalar> > &out, FFT::Direction dir, int device = 0)
    : _in(in), _out(out), _sign(dir == FFT::BACKWARD ? 1 : -1), _device(device) {
    if (in.size() != out.size()) {
      ConfigError err;
      err << "Can not construct FFT plan: input & output buffers are of different size!";
      throw err;
    }
    if (in.isEmpty() || out.isEmpty()) {
      ConfigError err;
      err << "Can not construct FFT plan: input or output buffer is empty!";
      throw err;
    }
    _make();
  }
  FFTPlan(const Buffer< std::complex<Scalar> > &inplace, FFT::Direction dir, int device = 0)
    : _in(inplace), _out(inplace), _sign(dir == FFT::BACKWARD ? 1 : -1), _device(device) {
    if (inplace.isEmpty()) {
      ConfigError err;
      err << "Can not construct FFT plan: Buffer is empty!";
      throw err;
    }
    _make();
  }
  virtual ~FFTPlan() {}
  /** Performs the transformation. */
  void operator() () {
    detail::configCheck(sdrhip_fft_plan_exec(_plan, _sign, _in.data(), _out.data()), "FFT plan");
  }
  /** Which device plan serves this size ("radix-16 lds", "lds", "four-step", "chirp", ...). */
  const char *form() const { const char *s = ""; sdrhip_fft_plan_form(_plan, &s); return s; }

protected:
  void _make() {
    if (_in.size() > (size_t(1) << 27)) {
      ConfigError err;
      err << "Can not construct FFT plan: " << _in.size() << " points exceed the device plans (2^27)";
      throw err;
    }
    detail::configCheck(sdrhip_fft_plan_create(Device::get(_device), detail::TypeTag< std::complex<Scalar> >::dtype, int(_in.size()), _plan.out()), "FFT plan");
  }
  Buffer< std::complex<Scalar> > _in, _out;
  int _sign, _device;
  detail::Handle<sdrhip_fft_plan, sdrhip_fft_plan_destroy> _plan;
};

}  // namespace gpu
}  // namespace sdr

#endif
