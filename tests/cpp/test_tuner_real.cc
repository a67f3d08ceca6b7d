// test_tuner_real.cc — sdr::gpu::RealTunerBank<int16_t> (include/sdr/gpu/nodes.hh): several BaseBand<int16_t> channels on one
// source of real int16 samples, as one node.
//   test_tuner_real --host-only      construction, config() rules, type checks, the no-device path (built under ASan/UBSan)
//   test_tuner_real <dir>            + the graph on the GPU: a source of <dir>/input.i16 in buffers of 4096 -> bank with a
//                                    demodulator per channel -> one Recorder per channel, against <dir>/row<c>.i16, the rows the
//                                    CPU oracle's BaseBand<int16_t> + demodulator made of the same buffers
//                                    (tests/test_cpp_tuner_real.py writes the files; TUNES, ORDER, D and FS are stated on both sides)
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "sdr/sdr.hh"

using namespace sdr;
typedef std::complex<int16_t> cs16;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

static const double FS = 2.0e6;
static const size_t BS = 4096, ORDER = 127, D = 20;

struct TuneSpec { double Fc, Ff, width; int mode; };
// NFM, an AM broadcast carrier, USB (the filter 1500 Hz above the carrier): fractions stay fractions in the real-input node
static const TuneSpec TUNES[] = {{101.5e3, 101.5e3, 12.5e3, SDRHIP_EPI_FM}, {455000.25, 455000.25, 9e3, SDRHIP_EPI_AM}, {14.07e3, 15.57e3, 3e3, SDRHIP_EPI_USB}};
static const size_t NT = 3;

template <class T> static std::vector<T> slurp(const std::string &path) {
  std::ifstream f(path.c_str(), std::ios::binary);
  std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  std::vector<T> v(raw.size() / sizeof(T));
  if (!v.empty()) memcpy(v.data(), raw.data(), v.size() * sizeof(T));
  return v;
}

struct Feeder : public Source {
  void cfg(Config::Type t, double fs, size_t bs) { setConfig(Config(t, fs, bs, 1)); }
  template <class T> void feed(T *p, size_t n) { Buffer<T> b(p, n); send(b, false); }
};
template <class T> struct Probe : public Recorder<T> {
  Config last;
  virtual void config(const Config &c) { last = c; }
};

template <class F> static bool throwsConfigError(F f) {
  try { f(); } catch (ConfigError &) { return true; }
  return false;
}

static void testHostOnly() {
  typedef gpu::RealTunerBank<int16_t> Bank;
  Bank bank(127, 8, SDRHIP_EPI_FM);
  Sink<int16_t> *as_sink = &bank; (void)as_sink;            // a Sink of real samples
  CHECK(bank.addChannel(100e3, 100e3, 50e3) == 0 && bank.addChannel(-300000.9, -300e3, 12500.5) == 1 && bank.channels() == 2);
  CHECK(bank.centerFrequency(1) == -300000.9 && bank.filterWidth(1) == 12500.5);   // doubles, as the reference's real-input node keeps them
  bank.setCenterFrequency(1, 99.9); bank.setFilterFrequency(1, -7.5); bank.setFilterWidth(0, 30000.99);
  CHECK(bank.centerFrequency(1) == 99.9 && bank.filterFrequency(1) == -7.5 && bank.filterWidth(0) == 30000.99);
  CHECK(!bank.perChannel() && bank.mode(0) == SDRHIP_EPI_FM && bank.source(0) != bank.source(1));
  CHECK(throwsConfigError([&] { bank.setMode(0, SDRHIP_EPI_AM); }) && throwsConfigError([&] { bank.addChannel(0, 0, 1e3, SDRHIP_EPI_USB); }));
  bank.config(Config());                                  // nothing known yet: silent
  bank.config(Config(Config::Type_s16, 0, 0, 1));         // no sample rate: still silent
  CHECK(throwsConfigError([&] { bank.config(Config(Config::Type_cs16, FS, BS, 1)); }));   // the complex bank's input type
  CHECK(throwsConfigError([&] { bank.config(Config(Config::Type_u8, FS, BS, 1)); }));
  // a demodulator per channel: the complex bank's rules
  Bank mixed(ORDER, D, Bank::PerChannel), raw(21, 8);
  CHECK(mixed.perChannel() && mixed.addChannel(1e3, 1e3, 3e3) == 0 && mixed.mode(0) == SDRHIP_EPI_FM);
  CHECK(mixed.addChannel(2e3, 2e3, 3e3, SDRHIP_EPI_USB) == 1 && mixed.mode(1) == SDRHIP_EPI_USB);
  mixed.setMode(0, SDRHIP_EPI_AM);
  CHECK(mixed.mode(0) == SDRHIP_EPI_AM);
  CHECK(throwsConfigError([&] { mixed.setMode(1, SDRHIP_EPI_NONE); }) && throwsConfigError([&] { mixed.addChannel(0, 0, 1e3, 7); }) && mixed.channels() == 2);
  CHECK(raw.addChannel(0, 0, 15e3) == 0 && raw.mode(0) == SDRHIP_EPI_NONE);
  // with a complete Config: a plan or a ConfigError (no device, no CPU fallback), never a crash
  try { bank.config(Config(Config::Type_s16, FS, BS, 1)); } catch (ConfigError &e) { (void)e; }
  try { mixed.config(Config(Config::Type_s16, FS, BS, 1)); } catch (ConfigError &e) { (void)e; }
  Feeder f; f.connect(&raw, true);
}

static void testGraphAgainstOracleRows(const std::string &dir) {
  std::vector<int16_t> x = slurp<int16_t>(dir + "/input.i16");
  CHECK(x.size() == 3 * BS + 1000);
  Feeder src;
  gpu::RealTunerBank<int16_t> bank(ORDER, D, gpu::RealTunerBank<int16_t>::PerChannel);
  std::vector<Probe<int16_t> > out(NT);
  for (size_t c = 0; c < NT; c++) CHECK(bank.addChannel(TUNES[c].Fc, TUNES[c].Ff, TUNES[c].width, TUNES[c].mode) == c);
  src.connect(&bank, true);
  for (size_t c = 0; c < NT; c++) bank.source(c)->connect(&out[c], true);
  src.cfg(Config::Type_s16, FS, BS);
  for (size_t c = 0; c < NT; c++)   // int16_t at Fs / D (the double quotient), buffers of ceil(BS / D) + 1
    CHECK(out[c].last.type() == Config::Type_s16 && out[c].last.sampleRate() == FS / double(D) && out[c].last.bufferSize() == (BS + D - 1) / D + 1);
  // three whole buffers and a short one: windows of D samples from the first sample on stay open across them
  const size_t cuts[] = {BS, BS, BS, 1000};
  const size_t lens[] = {204, 205, 205, 50};   // 4096 = 204 * 20 + 16, ...
  size_t off = 0;
  for (size_t b = 0; b < 4; b++) { src.feed(x.data() + off, cuts[b]); off += cuts[b]; }
  for (size_t c = 0; c < NT; c++) {
    char name[32];
    std::snprintf(name, sizeof name, "/row%zu.i16", c);
    const std::vector<int16_t> want = slurp<int16_t>(dir + name);
    CHECK(want.size() == 664);
    CHECK(out[c].lens == std::vector<size_t>(lens, lens + 4));
    CHECK(out[c].data == want);
  }
  // the three rows are three different demodulators' work
  CHECK(out[0].data != out[1].data && out[1].data != out[2].data);
}

int main(int argc, char **argv) {
  const bool host_only = argc > 1 && std::string(argv[1]) == "--host-only";
  Logger::get().addHandler(new StreamLogHandler(std::cerr, LOG_ERROR));
  try {
    testHostOnly();
    if (!host_only) {
      if (argc < 2) { std::printf("usage: test_tuner_real --host-only | <dir>\n"); return 2; }
      testGraphAgainstOracleRows(argv[1]);
    }
  } catch (std::exception &e) { std::printf("FAIL: exception: %s\n", e.what()); return 2; }
  std::printf("%s (%d failures)\n", failures ? "FAILED" : "OK", failures);
  return failures ? 1 : 0;
}
