// test_receiver_bank.cc — sdr::gpu::ReceiverBank<int16_t> (include/sdr/gpu/receiver.hh): one antenna to every channel's bits.
//   test_receiver_bank --host-only   construction, services kept, config() rules, type / mode / service checks, the no-device
//                                    path, destructors (built under ASan/UBSan)
//   test_receiver_bank <dir>         + the five-channel plan in a graph on the GPU: a source of <dir>/input.cs16 cut into the
//                                    plan's 13 buffers -> ReceiverBank -> one bit recorder and one audio recorder per channel,
//                                    against <dir>/bits<c>.u8, bits<c>.lens, audio<c>.i16, audio<c>.lens — what the CPU
//                                    references made of the same buffers (tests/test_cpp_receiver.py writes the files;
//                                    the plan is stated on both sides, tests/receiver_plan.py)
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "sdr/sdr.hh"
#include "sdr/gpu/receiver.hh"

using namespace sdr;
typedef std::complex<int16_t> cs16;
typedef gpu::ReceiverBank<int16_t> Rx;
typedef Rx::Service Service;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

static const double FS = 176400.0;
static const size_t BS = 8192, ORDER = 21, D = 8, M = 1024;
static const size_t LENS[] = {8192, 8192, 8192, 8192, 8192, 1000, 0, 1, 7, 513, 4095, 8192, 8192};
static const size_t NCALLS = sizeof(LENS) / sizeof(LENS[0]);

struct ChannelSpec { double Fc, Ff, width; int mode; Service service; };
static std::vector<ChannelSpec> plan() {
  const gpu::BitStream::Mode N = gpu::BitStream::NORMAL, T = gpu::BitStream::TRANSITION;
  std::vector<ChannelSpec> p;
  p.push_back(ChannelSpec{30e3, 30e3, 12.5e3, SDRHIP_EPI_FM, Service::fsk(1200.f, 1200.f, 2200.f, T, true)});
  p.push_back(ChannelSpec{-42e3, -42e3, 12.5e3, SDRHIP_EPI_FM, Service::ask(1200.f, false, N, false)});
  p.push_back(ChannelSpec{61e3, 62e3, 2.5e3, SDRHIP_EPI_USB, Service::fsk(90.90f, 930.f, 1100.f, N, false)});
  p.push_back(ChannelSpec{-15e3, -15e3, 9e3, SDRHIP_EPI_AM, Service::fsk(1200.f, 1200.f, 2200.f, N, false)});
  p.push_back(ChannelSpec{75e3, 75e3, 12.5e3, SDRHIP_EPI_FM, Service::fsk(1200.f, 1200.f, 2200.f, T, true)});
  return p;
}

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
  const std::vector<ChannelSpec> p = plan();
  {
    Rx rx(ORDER, D);
    Sink<cs16> *as_sink = &rx; (void)as_sink;
    for (size_t c = 0; c < p.size(); c++) CHECK(rx.addChannel(p[c].Fc, p[c].Ff, p[c].width, p[c].mode, p[c].service) == c);
    CHECK(rx.channels() == 5 && rx.perChannel());
    // services, modes and tunes are kept as given
    CHECK(rx.service(0).kind == Service::FSK && rx.service(0).baud == 1200.f && rx.service(0).mark == 1200.f && rx.service(0).space == 2200.f);
    CHECK(rx.service(0).mode == gpu::BitStream::TRANSITION && rx.service(0).deemph);
    CHECK(rx.service(1).kind == Service::ASK && !rx.service(1).invert && rx.service(1).mode == gpu::BitStream::NORMAL && !rx.service(1).deemph);
    CHECK(rx.service(2).baud == 90.90f && rx.mode(2) == SDRHIP_EPI_USB && rx.mode(3) == SDRHIP_EPI_AM && rx.mode(4) == SDRHIP_EPI_FM);
    CHECK(rx.centerFrequency(2) == 61e3 && rx.filterFrequency(2) == 62e3 && rx.filterWidth(2) == 2500);
    CHECK(rx.bits(0) != rx.bits(1) && rx.audio(0) != rx.audio(1) && rx.bits(0) != rx.audio(0));
    // before config() the setters only record
    rx.setService(1, Service::ask(300.f, true, gpu::BitStream::TRANSITION, true));
    CHECK(rx.service(1).invert && rx.service(1).baud == 300.f && rx.service(1).deemph);
    rx.enableDeemph(1, false); rx.setMode(3, SDRHIP_EPI_FM); rx.setCenterFrequency(4, 74200.7);
    CHECK(!rx.service(1).deemph && rx.mode(3) == SDRHIP_EPI_FM && rx.centerFrequency(4) == 74200);   // (IQBaseBand keeps int32)
    // a bad mode or service: ConfigError, and nothing is added or changed
    Service bad = Service::fsk(0.f, 1200.f, 2200.f);
    CHECK(throwsConfigError([&] { rx.addChannel(0, 0, 1e3, SDRHIP_EPI_FM, bad); }));
    CHECK(throwsConfigError([&] { rx.addChannel(0, 0, 1e3, SDRHIP_EPI_NONE, p[0].service); }));
    CHECK(throwsConfigError([&] { rx.addChannel(0, 0, 1e3, 7, p[0].service); }));
    CHECK(throwsConfigError([&] { rx.setService(0, bad); }));
    bad = Service::ask(-1200.f);
    CHECK(throwsConfigError([&] { rx.setService(0, bad); }));
    CHECK(throwsConfigError([&] { rx.setMode(0, SDRHIP_EPI_NONE); }));
    CHECK(rx.channels() == 5 && rx.service(0).kind == Service::FSK && rx.service(0).mode == gpu::BitStream::TRANSITION);
    // Config rules: silent while incomplete, ConfigError on a wrong input type
    rx.config(Config());
    rx.config(Config(Config::Type_cs16, 0, 0, 1));
    CHECK(throwsConfigError([&] { rx.config(Config(Config::Type_s16, FS, BS, 1)); }));
    CHECK(throwsConfigError([&] { rx.config(Config(Config::Type_cu8, FS, BS, 1)); }));
    // with a complete Config: a plan or a ConfigError (no device, no CPU fallback), never a crash
    try { rx.config(Config(Config::Type_cs16, FS, BS, 1)); } catch (ConfigError &e) { (void)e; }
    try { rx.addChannel(1e3, 1e3, 3e3, SDRHIP_EPI_AM, Service::ask(1200.f)); } catch (ConfigError &e) { (void)e; }
    std::vector<cs16> zeros(16);
    Feeder f; f.connect(&rx, true);
    Probe<uint8_t> b0; rx.bits(0)->connect(&b0, true);
    try { f.feed(zeros.data(), zeros.size()); } catch (ConfigError &e) { (void)e; }
  }
  { Rx empty(ORDER, D); empty.config(Config(Config::Type_cs16, FS, BS, 1)); }   // no channel: no plan, nothing to release
}

static void testGraphAgainstReferenceFiles(const std::string &dir) {
  const std::vector<ChannelSpec> p = plan();
  const size_t C = p.size();
  std::vector<cs16> x = slurp<cs16>(dir + "/input.cs16");
  size_t total = 0;
  for (size_t k = 0; k < NCALLS; k++) total += LENS[k];
  CHECK(x.size() == total);
  Feeder src;
  Rx rx(ORDER, D);
  std::vector<Probe<uint8_t> > bits(C);
  std::vector<Probe<int16_t> > audio(C);
  for (size_t c = 0; c < C; c++) CHECK(rx.addChannel(p[c].Fc, p[c].Ff, p[c].width, p[c].mode, p[c].service) == c);
  src.connect(&rx, true);
  for (size_t c = 0; c < C; c++) { rx.bits(c)->connect(&bits[c], true); rx.audio(c)->connect(&audio[c], true); }
  src.cfg(Config::Type_cs16, FS, BS);
  for (size_t c = 0; c < C; c++) {
    // bits(c) as gpu::BitStream configures its own: uint8 at the baud rate, buffers of that channel's capacity
    const double omax = double(float(double(float(p[c].service.baud / 22050.0)) * 1.005));
    CHECK(bits[c].last.type() == Config::Type_u8 && bits[c].last.sampleRate() == double(p[c].service.baud));
    CHECK(bits[c].last.bufferSize() >= size_t(M * omax) && bits[c].last.bufferSize() <= size_t(M * omax) + 2);
    CHECK(audio[c].last.type() == Config::Type_s16 && audio[c].last.sampleRate() == 22050.0 && audio[c].last.bufferSize() == M + 1);
  }
  size_t off = 0;
  for (size_t k = 0; k < NCALLS; k++) { src.feed(x.data() + off, LENS[k]); off += LENS[k]; }
  for (size_t c = 0; c < C; c++) {
    char name[64];
    std::snprintf(name, sizeof name, "/bits%zu", c);
    const std::vector<uint8_t> wb = slurp<uint8_t>(dir + name + ".u8");
    const std::vector<uint32_t> wbl = slurp<uint32_t>(dir + name + ".lens");
    std::snprintf(name, sizeof name, "/audio%zu", c);
    const std::vector<int16_t> wa = slurp<int16_t>(dir + name + ".i16");
    const std::vector<uint32_t> wal = slurp<uint32_t>(dir + name + ".lens");
    CHECK(!wb.empty() && !wa.empty());
    CHECK(bits[c].lens == std::vector<size_t>(wbl.begin(), wbl.end()));     // buffer by buffer; a buffer without bits sent nothing
    CHECK(bits[c].data == wb);
    CHECK(audio[c].lens == std::vector<size_t>(wal.begin(), wal.end()));
    CHECK(audio[c].data == wa);
    for (size_t i = 0; i < bits[c].lens.size(); i++) CHECK(bits[c].lens[i] > 0);
    CHECK(bits[c].lens.size() < NCALLS - 1);
  }
}

int main(int argc, char **argv) {
  const bool host_only = argc > 1 && std::string(argv[1]) == "--host-only";
  Logger::get().addHandler(new StreamLogHandler(std::cerr, LOG_ERROR));
  try {
    testHostOnly();
    if (!host_only) {
      if (argc < 2) { std::printf("usage: test_receiver_bank --host-only | <dir>\n"); return 2; }
      testGraphAgainstReferenceFiles(argv[1]);
    }
  } catch (std::exception &e) { std::printf("FAIL: exception: %s\n", e.what()); return 2; }
  std::printf("%s (%d failures)\n", failures ? "FAILED" : "OK", failures);
  return failures ? 1 : 0;
}
