// test_tuner.cc — sdr::gpu::TunerBank<int16_t> (include/sdr/gpu/nodes.hh) in graphs of this repository's sdr:: core: one
// source -> bank -> one Recorder per channel, against the g4_iqbb127d8_fm fixture cut from the reference and against
// separate gpu::IQBaseBand<int16_t> + gpu::FMDemod<int16_t> pairs connected to the same source.
//   test_tuner --host-only <golden>   config() rules, no device needed (built under ASan/UBSan)
//   test_tuner <golden>               + the graphs on the GPU
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "sdr/sdr.hh"

using namespace sdr;
typedef std::complex<int16_t> cs16;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

static std::string g_golden = "tests/golden";
static const double FS = 2.4e6;
static const size_t BS = 4096;

template <class T> static std::vector<T> slurp(const std::string &name) {
  std::ifstream f((g_golden + "/" + name).c_str(), std::ios::binary);
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

struct TuneSpec { double Fc, Ff, width; };
// channel 0: the g4_iqbb127d8_fm tune; both signs, no shift, and tunes with fractions (the reference node keeps int32 members)
static const TuneSpec TUNES[] = {{100e3, 100e3, 50e3}, {-300e3, -300e3, 50e3}, {0, 20e3, 30e3}, {100000.9, 100000.7, 12500.5},
                                 {-250000.6, -249999.5, 80000.9}};
static const size_t NT = sizeof(TUNES) / sizeof(TUNES[0]);

static void testHostOnly() {
  gpu::TunerBank<int16_t> bank(127, 8, SDRHIP_EPI_FM);
  CHECK(bank.addChannel(100e3, 100e3, 50e3) == 0 && bank.addChannel(-300000.9, -300e3, 12500.5) == 1 && bank.channels() == 2);
  CHECK(bank.centerFrequency(1) == -300000.0 && bank.filterWidth(1) == 12500.0);   // truncated as the reference's members
  bank.setCenterFrequency(1, 99.9); bank.setFilterFrequency(1, -7.5); bank.setFilterWidth(0, 30000.99);
  CHECK(bank.centerFrequency(1) == 99.0 && bank.filterFrequency(1) == -7.0 && bank.filterWidth(0) == 30000.0);
  bank.config(Config());                                  // nothing known yet: silent
  bank.config(Config(Config::Type_cs16, 0, 0, 1));        // no sample rate: still silent
  bool threw = false;
  try { bank.config(Config(Config::Type_s16, FS, BS, 1)); } catch (ConfigError &) { threw = true; }
  CHECK(threw);                                           // a wrong input type
  try { bank.config(Config(Config::Type_cs16, FS, BS, 1)); } catch (ConfigError &e) { (void)e; }   // without a device: a ConfigError, never a crash
  Feeder f; f.connect(&bank, true);
}

static void testAgainstFixtureAndPairs() {
  std::vector<cs16> x = slurp<cs16>("g1_iq_cs16.bin");
  const std::vector<int16_t> want = slurp<int16_t>("g4_iqbb127d8_fm.bin");
  CHECK(x.size() == 4 * BS && want.size() == 2047);
  Feeder src;
  gpu::TunerBank<int16_t> bank(127, 8, SDRHIP_EPI_FM);
  std::vector<std::unique_ptr<gpu::IQBaseBand<int16_t> > > bb;
  std::vector<std::unique_ptr<gpu::FMDemod<int16_t> > > fm;
  std::vector<Probe<int16_t> > out(NT), ref(NT);
  for (size_t c = 0; c < NT; c++) {
    CHECK(bank.addChannel(TUNES[c].Fc, TUNES[c].Ff, TUNES[c].width) == c);
    bb.emplace_back(new gpu::IQBaseBand<int16_t>(TUNES[c].Fc, TUNES[c].Ff, TUNES[c].width, 127, 8));
    fm.emplace_back(new gpu::FMDemod<int16_t>());
  }
  src.connect(&bank, true);
  for (size_t c = 0; c < NT; c++) {
    bank.source(c)->connect(&out[c], true);
    src.connect(bb[c].get(), true); bb[c]->connect(fm[c].get(), true); fm[c]->connect(&ref[c], true);
  }
  src.cfg(Config::Type_cs16, FS, BS);
  for (size_t c = 0; c < NT; c++) {   // type, rate, buffer size per source
    CHECK(out[c].last.type() == Config::Type_s16 && out[c].last.sampleRate() == 300000.0 && out[c].last.bufferSize() == BS / 8 + 1);
    CHECK(bank.source(c)->type() == Config::Type_s16);
  }
  for (size_t b = 0; b < 4; b++) {
    if (b == 2) {   // retune ONE channel between buffers, with a fraction: bank and pair alike
      bank.setCenterFrequency(1, -150000.9); bb[1]->setCenterFrequency(-150000.9);
      bank.setFilterFrequency(3, 90000.5); bb[3]->setFilterFrequency(90000.5);
      bank.setFilterWidth(4, 20000.7); bb[4]->setFilterWidth(20000.7);
    }
    src.feed(&x[b * BS], BS);
  }
  CHECK(out[0].data == want);
  const size_t lens[] = {511, 512, 512, 512};
  for (size_t c = 0; c < NT; c++) {
    CHECK(out[c].lens == std::vector<size_t>(lens, lens + 4));
    CHECK(out[c].data == ref[c].data);
    if (c) CHECK(out[c].data != out[0].data);
  }
}

// the bank's outputs are views of one stage buffer: while a consumer still references a view of the last round, the next
// buffer is dropped (reference src/baseband.hh:141-150), and the held view is not clobbered
static void testDropsWhileOutputInUse() {
  struct Hold : public Sink<cs16> {
    RawBuffer kept; bool keep = false; size_t calls = 0; std::vector<cs16> first;
    virtual void config(const Config &) {}
    virtual void process(const Buffer<cs16> &b, bool) {
      calls++;
      if (keep) { kept = b; kept.ref(); first.assign(reinterpret_cast<const cs16 *>(b.data()), reinterpret_cast<const cs16 *>(b.data()) + b.size()); }
    }
  };
  std::vector<cs16> x = slurp<cs16>("g1_iq_cs16.bin");
  Feeder src;
  gpu::TunerBank<int16_t> bank(21, 8);
  std::vector<Hold> hold(3);
  for (size_t c = 0; c < 3; c++) { bank.addChannel(TUNES[c].Fc, TUNES[c].Ff, TUNES[c].width); bank.source(c)->connect(&hold[c], true); }
  src.connect(&bank, true);
  src.cfg(Config::Type_cs16, FS, BS);
  hold[1].keep = true;
  src.feed(&x[0], BS);
  CHECK(hold[0].calls == 1 && hold[1].calls == 1 && hold[2].calls == 1 && hold[1].first.size() == 511);
  hold[1].keep = false;
  src.feed(&x[BS], BS);                                    // view of round 1 still referenced -> dropped
  CHECK(hold[0].calls == 1 && hold[2].calls == 1);
  CHECK(0 == memcmp(hold[1].kept.data(), hold[1].first.data(), hold[1].first.size() * sizeof(cs16)));
  hold[1].kept.unref();
  src.feed(&x[2 * BS], BS);
  CHECK(hold[0].calls == 2 && hold[2].calls == 2);
}

// addChannel after config(): the plan is rebuilt, every channel restarts as a freshly configured node
static void testAddChannelAfterConfig() {
  std::vector<cs16> x = slurp<cs16>("g1_iq_cs16.bin");
  Feeder src, src2;
  gpu::TunerBank<int16_t> bank(33, 5, SDRHIP_EPI_USB), fresh(33, 5, SDRHIP_EPI_USB);
  std::vector<Probe<int16_t> > out(3), want(3);
  for (size_t c = 0; c < 2; c++) { bank.addChannel(TUNES[c].Fc, TUNES[c].Ff, TUNES[c].width); bank.source(c)->connect(&out[c], true); }
  src.connect(&bank, true);
  src.cfg(Config::Type_cs16, FS, BS);
  src.feed(&x[0], 1000);
  CHECK(out[0].lens.size() == 1 && out[0].lens[0] == 199);
  CHECK(bank.addChannel(TUNES[2].Fc, TUNES[2].Ff, TUNES[2].width) == 2);
  bank.source(2)->connect(&out[2], true);
  CHECK(out[2].last.type() == Config::Type_s16 && out[2].last.sampleRate() == 480000.0 && out[2].last.bufferSize() == (BS + 4) / 5 + 1);
  for (size_t c = 0; c < 3; c++) { out[c].data.clear(); out[c].lens.clear(); }
  src.feed(&x[1000], 3000);
  for (size_t c = 0; c < 3; c++) { fresh.addChannel(TUNES[c].Fc, TUNES[c].Ff, TUNES[c].width); fresh.source(c)->connect(&want[c], true); }
  src2.connect(&fresh, true);
  src2.cfg(Config::Type_cs16, FS, BS);
  src2.feed(&x[1000], 3000);
  for (size_t c = 0; c < 3; c++) CHECK(!out[c].data.empty() && out[c].data == want[c].data);
}

int main(int argc, char **argv) {
  bool host_only = false;
  int a = 1;
  if (argc > a && std::string(argv[a]) == "--host-only") { host_only = true; a++; }
  if (argc > a) g_golden = argv[a];
  Logger::get().addHandler(new StreamLogHandler(std::cerr, LOG_ERROR));
  try {
    testHostOnly();
    if (!host_only) {
      testAgainstFixtureAndPairs();
      testDropsWhileOutputInUse();
      testAddChannelAfterConfig();
    }
  } catch (std::exception &e) { std::printf("FAIL: exception: %s\n", e.what()); return 2; }
  std::printf("%s (%d failures)\n", failures ? "FAILED" : "OK", failures);
  return failures ? 1 : 0;
}
