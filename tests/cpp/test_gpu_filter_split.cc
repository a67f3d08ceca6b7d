// test_gpu_filter_split.cc — gpu::FilterSink / gpu::FilterSource (include/sdr/gpu/nodes.hh) in graphs on this repository's
// sdr:: core: the device hand-off, host spectra both ways, config errors, and FilterNode's bands as FilterSources. Compared
// with the CPU oracle's overlap-add filter (oracle/sdr_oracle.h). Needs an MI355X.
#include <cstdio>
#include <complex>
#include <vector>

#include "sdr/sdr.hh"
#include "sdr_oracle.h"

using namespace sdr;
typedef std::complex<float> cf32;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

static const double FS = 2.4e6;
static const size_t N = 1024, NB = 4;

struct Feeder : public Source {
  void cfg(Config::Type t, size_t bs) { setConfig(Config(t, FS, bs, 1)); }
  template <class T> void feed(T *p, size_t n) { Buffer<T> b(p, n); send(b, false); }
};

struct CfgProbe : public Sink<cf32> {
  size_t bs = 0;
  virtual void config(const Config &c) { bs = c.bufferSize(); }
  virtual void process(const Buffer<cf32> &, bool) {}
};

static std::vector<cf32> input() {
  IQSigGen<float> gen(FS, N); gen.addSine(100e3, 0.5, 0.0); gen.addSine(-300e3, 0.3, 0.3);
  Recorder<cf32> r; gen.connect(&r, true);
  for (size_t b = 0; b < NB; b++) gen.next();
  return r.data;
}

// the oracle's FilterSink + FilterSource over NB blocks
static std::vector<cf32> oracle(const std::vector<cf32> &x, double fmin, double fmax) {
  std::vector<float> h(2 * N), K(4 * N);
  orc_fftfilt_design_h(int(N), fmin, fmax, FS, h.data());
  orc_fftfilt_design_K(int(N), h.data(), K.data());
  void *f = orc_fftfilt_create(int(N), K.data());
  std::vector<cf32> y(x.size());
  for (size_t b = 0; b < x.size() / N; b++) orc_fftfilt_process(f, (const float *)(x.data() + b * N), (float *)(y.data() + b * N));
  orc_fftfilt_destroy(f);
  return y;
}

static double relErr(const std::vector<cf32> &a, const std::vector<cf32> &b) {
  if (a.size() != b.size() || a.empty()) return 1e30;
  double e = 0, m = 0;
  for (size_t i = 0; i < a.size(); i++) { e = std::max(e, (double)std::abs(a[i] - b[i])); m = std::max(m, (double)std::abs(b[i])); }
  return e / m;
}

// the 2N-point DFT of each zero-padded block, in double
static double spectrumErr(const std::vector<cf32> &x, const std::vector<cf32> &spec) {
  if (spec.size() != 2 * x.size()) return 1e30;
  double e = 0, m = 0;
  const size_t L = 2 * N;
  for (size_t b = 0; b < x.size() / N; b++)
    for (size_t k = 0; k < L; k += 37) {   // a sample of the bins
      std::complex<double> s = 0;
      for (size_t n = 0; n < N; n++) s += std::complex<double>(x[b * N + n]) * std::polar(1.0, -2 * M_PI * double((k * n) % L) / double(L));
      e = std::max(e, std::abs(s - std::complex<double>(spec[b * L + k]))); m = std::max(m, std::abs(s));
    }
  return e / m;
}

static void testDeviceHandoff(const std::vector<cf32> &x) {
  Feeder src; gpu::FilterSink<float> sink(N); gpu::FilterSource<float> a(N, 50e3, 150e3), b(N, -350e3, -250e3);
  Recorder<cf32> ra, rb;
  src.connect(&sink, true); sink.connect(&a, true); sink.connect(&b, true); a.connect(&ra, true); b.connect(&rb, true);
  src.cfg(Config::Type_cf32, N);
  for (size_t k = 0; k < NB; k++) src.feed(const_cast<cf32 *>(x.data() + k * N), N);
  CHECK(sink.lastBlockOnDevice() && a.lastBlockOnDevice() && b.lastBlockOnDevice());
  CHECK(relErr(ra.data, oracle(x, 50e3, 150e3)) <= 1e-5);
  CHECK(relErr(rb.data, oracle(x, -350e3, -250e3)) <= 1e-5);
}

static void testHostSpectra(const std::vector<cf32> &x) {
  Feeder src; gpu::FilterSink<float> sink(N); Recorder<cf32> spec; CfgProbe probe;
  src.connect(&sink, true); sink.connect(&spec, true); sink.connect(&probe, true);
  src.cfg(Config::Type_cf32, N);
  CHECK(probe.bs == N);   // the reference propagates N, though its buffers hold 2N
  for (size_t k = 0; k < NB; k++) src.feed(const_cast<cf32 *>(x.data() + k * N), N);
  CHECK(!sink.lastBlockOnDevice());
  CHECK(spec.lens.size() == NB && spec.lens[0] == 2 * N);
  CHECK(spectrumErr(x, spec.data) <= 1e-5);
  // a host spectrum source -> gpu::FilterSource: uploads
  Feeder hs; gpu::FilterSource<float> f(N, 50e3, 150e3); Recorder<cf32> out;
  hs.connect(&f, true); f.connect(&out, true);
  hs.cfg(Config::Type_cf32, N);
  for (size_t k = 0; k < NB; k++) hs.feed(spec.data.data() + k * 2 * N, 2 * N);
  CHECK(!f.lastBlockOnDevice());
  CHECK(relErr(out.data, oracle(x, 50e3, 150e3)) <= 1e-5);
}

static void testMixedFanOut(const std::vector<cf32> &x) {
  Feeder src; gpu::FilterSink<float> sink(N); gpu::FilterSource<float> a(N, 50e3, 150e3); Recorder<cf32> spec, ra;
  src.connect(&sink, true); sink.connect(&a, true); sink.connect(&spec, true); a.connect(&ra, true);
  src.cfg(Config::Type_cf32, N);
  for (size_t k = 0; k < NB; k++) src.feed(const_cast<cf32 *>(x.data() + k * N), N);
  CHECK(!sink.lastBlockOnDevice() && !a.lastBlockOnDevice());
  CHECK(relErr(ra.data, oracle(x, 50e3, 150e3)) <= 1e-5);
  CHECK(spectrumErr(x, spec.data) <= 1e-5);
}

static void testConfigErrors() {
  bool thrown = false;
  try { Feeder s; gpu::FilterSink<float> k(N); s.connect(&k, true); s.cfg(Config::Type_cf32, N / 2); }
  catch (ConfigError &) { thrown = true; }
  CHECK(thrown);
  thrown = false;
  try { Feeder s; gpu::FilterSink<float> k(N); s.connect(&k, true); s.cfg(Config::Type_cf64, N); }
  catch (ConfigError &) { thrown = true; }
  CHECK(thrown);
  thrown = false;
  try { Feeder s; gpu::FilterSource<float> f(N, 0, 1e5); s.connect(&f, true); s.cfg(Config::Type_cf32, 2 * N); }
  catch (ConfigError &) { thrown = true; }
  CHECK(thrown);
}

// FilterNode's bands are gpu::FilterSources: setFreq through the base pointer reaches the bank
static void testBankBase(const std::vector<cf32> &x) {
  std::vector<cf32> outs[2];
  for (int via_base = 0; via_base < 2; via_base++) {
    Feeder src; gpu::FilterNode<float> bank(N); Recorder<cf32> r;
    src.connect(bank.sink(), true);
    gpu::FilterNode<float>::Band *band = bank.addFilter(50e3, 150e3);
    gpu::FilterSource<float> *s = bank.addFilter(-350e3, -250e3);
    s->connect(&r, true);
    (void)band;
    src.cfg(Config::Type_cf32, N);
    src.feed(const_cast<cf32 *>(x.data()), N);
    if (via_base) s->setFreq(100e3, 200e3);
    else static_cast<gpu::FilterNode<float>::Band *>(s)->setFreq(100e3, 200e3);
    CHECK(s->fmin() == 100e3 && s->fmax() == 200e3);
    for (size_t k = 1; k < NB; k++) src.feed(const_cast<cf32 *>(x.data() + k * N), N);
    outs[via_base] = r.data;
  }
  CHECK(outs[0].size() == NB * N && outs[0] == outs[1]);
}

int main() {
  const std::vector<cf32> x = input();
  testDeviceHandoff(x);
  testHostSpectra(x);
  testMixedFanOut(x);
  testConfigErrors();
  testBankBase(x);
  std::printf("%s (%d failures)\n", failures ? "FAILED" : "OK", failures);
  return failures ? 1 : 0;
}
