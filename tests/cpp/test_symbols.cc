// test_symbols.cc — sdr::gpu::FSKDetector, ASKDetector<int16_t> and BitStream (include/sdr/gpu/nodes.hh) in graphs of this
// repository's sdr:: core against the g18 fixtures cut from the reference (tests/golden/manifest_fsk.json).
//   test_symbols --host-only <golden>   config() rules and the designer, no device needed
//   test_symbols <golden>               + sdr_ax25's graph detector -> bits -> Recorder on the GPU
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "sdr/sdr.hh"

using namespace sdr;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

static std::string g_golden = "tests/golden";
static const double FS = 22050.0;

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
struct ConfigProbe : public Sink<uint8_t> {
  Config last;
  virtual void config(const Config &c) { last = c; }
  virtual void process(const Buffer<uint8_t> &, bool) {}
};

template <class Node> static void configRules(Node &n, Config::Type good, Config::Type bad, const char *what) {
  n.config(Config());                                  // nothing known yet: silent
  n.config(Config(good, 0, 0, 1));                     // no sample rate: still silent
  bool threw = false;
  try { n.config(Config(bad, FS, 4096, 1)); } catch (ConfigError &) { threw = true; }
  if (!threw) std::printf("  %s accepted a wrong input type\n", what);
  CHECK(threw);
  try { n.config(Config(good, FS, 4096, 1)); } catch (ConfigError &e) { (void)e; }   // without a device: a ConfigError, never a crash
}

static void testHostOnly() {
  CHECK(gpu::design::fskCorrLen(FS, 1200.f) == 18 && gpu::design::fskCorrLen(FS, 90.90f) == 242);
  const float tones[2][3] = {{1200.f, 1200.f, 2200.f}, {90.90f, 930.f, 1100.f}};
  const char *names[2] = {"g18_ax25", "g18_rtty"};
  for (int k = 0; k < 2; k++) {
    const int L = gpu::design::fskCorrLen(FS, tones[k][0]);
    std::vector<float> m(2 * L), s(2 * L);
    gpu::design::fskLut(FS, tones[k][1], L, m.data());
    gpu::design::fskLut(FS, tones[k][2], L, s.data());
    const std::vector<float> wm = slurp<float>(std::string(names[k]) + "_lut_mark.bin"), ws = slurp<float>(std::string(names[k]) + "_lut_space.bin");
    CHECK(wm.size() == m.size() && 0 == memcmp(wm.data(), m.data(), m.size() * sizeof(float)));
    CHECK(ws.size() == s.size() && 0 == memcmp(ws.data(), s.data(), s.size() * sizeof(float)));
  }
  { gpu::FSKDetector n(1200, 1200, 2200); configRules(n, Config::Type_s16, Config::Type_cs16, "FSKDetector"); }
  { gpu::ASKDetector<int16_t> n(true); configRules(n, Config::Type_s16, Config::Type_u8, "ASKDetector"); }
  { gpu::BitStream n(1200, gpu::BitStream::NORMAL); configRules(n, Config::Type_u8, Config::Type_s16, "BitStream"); }
}

static void runAx25(gpu::BitStream::Mode mode, const char *tag, bool viaProbe) {
  std::vector<int16_t> x = slurp<int16_t>("g18_ax25_x.bin");
  const size_t lens[] = {4096, 1000, 1, 17, 3078, 0, 2048};
  Feeder src;
  gpu::FSKDetector det(1200, 1200, 2200);
  gpu::BitStream bits(1200, mode);
  Recorder<uint8_t> sym, out;
  src.connect(&det, true);
  if (viaProbe) det.connect(&sym, true);     // a second, host-side sink: the symbols are copied into the buffer
  det.connect(&bits, true);
  bits.connect(&out, true);
  src.cfg(Config::Type_s16, FS, 8192);
  CHECK(det.Source::type() == Config::Type_u8 && det.Source::sampleRate() == FS && bits.Source::type() == Config::Type_u8 && bits.Source::sampleRate() == 1200.0);
  std::vector<int32_t> counts;
  size_t off = 0;
  for (size_t b = 0; b < sizeof(lens) / sizeof(lens[0]); b++) {
    const size_t before = out.data.size(), sends = out.lens.size();
    src.feed(x.data() + off, lens[b]);
    off += lens[b];
    counts.push_back(int32_t(out.data.size() - before));
    CHECK((out.lens.size() == sends) == (out.data.size() == before));     // nothing is sent for a bit-less buffer ...
    if (lens[b] <= 1) CHECK(out.lens.size() == sends);                      // ... such as the empty and the 1-sample one
    CHECK(det.lastBufferOnDevice() == !viaProbe && bits.lastBufferOnDevice() == !viaProbe);
  }
  CHECK(out.data == slurp<uint8_t>(std::string("g18_ax25_bits_") + tag + ".bin"));
  CHECK(counts == slurp<int32_t>(std::string("g18_ax25_bits_") + tag + "_counts.bin"));
  if (viaProbe) CHECK(sym.data == slurp<uint8_t>("g18_ax25_sym.bin"));
}

static void testAsk() {
  std::vector<int16_t> x = slurp<int16_t>("g18_ask_x.bin");
  for (int inv = 0; inv < 2; inv++) {
    Feeder src;
    gpu::ASKDetector<int16_t> det(inv != 0);
    gpu::BitStream bits(1200, gpu::BitStream::NORMAL);
    Recorder<uint8_t> sym, out;
    src.connect(&det, true); det.connect(&sym, true); det.connect(&bits, true); bits.connect(&out, true);
    src.cfg(Config::Type_s16, FS, 8192);
    const size_t lens[] = {4096, 1000, 1, 17, 3078, 0};
    size_t off = 0;
    for (size_t b = 0; b < 6; b++) { src.feed(x.data() + off, lens[b]); off += lens[b]; }
    const std::string t = inv ? "g18_ask_inv1" : "g18_ask_inv0";
    CHECK(sym.data == slurp<uint8_t>(t + "_sym.bin") && out.data == slurp<uint8_t>(t + "_bits_normal.bin"));
  }
}

static void testReconfig() {
  // a changed source Config runs config() down the chain: both nodes start over (g18_reconf, before buffer 2)
  std::vector<int16_t> x = slurp<int16_t>("g18_reconf_x.bin");
  Feeder src;
  gpu::FSKDetector det(1200, 1200, 2200);
  gpu::BitStream bits(1200, gpu::BitStream::TRANSITION);
  ConfigProbe probe;
  Recorder<uint8_t> out;
  src.connect(&det, true); det.connect(&bits, true); bits.connect(&out, true); bits.connect(&probe, true);
  src.cfg(Config::Type_s16, FS, 8192);
  const size_t lens[] = {3000, 1111, 2000, 2081};
  size_t off = 0;
  for (size_t b = 0; b < 4; b++) {
    if (b == 2) src.cfg(Config::Type_s16, FS, 4096);
    src.feed(x.data() + off, lens[b]);
    off += lens[b];
  }
  CHECK(out.data == slurp<uint8_t>("g18_reconf_bits_transition.bin"));
  CHECK(probe.last.type() == Config::Type_u8 && probe.last.sampleRate() == 1200.0 && probe.last.bufferSize() == 226);   // ceil(4096 omegaMax) + 1
}

int main(int argc, char **argv) {
  bool host_only = false;
  int a = 1;
  if (argc > a && std::string(argv[a]) == "--host-only") { host_only = true; a++; }
  if (argc > a) g_golden = argv[a];
  Logger::get().addHandler(new StreamLogHandler(std::cerr, LOG_WARNING));
  try {
    testHostOnly();
    if (!host_only) {
      runAx25(gpu::BitStream::TRANSITION, "transition", false);
      runAx25(gpu::BitStream::NORMAL, "normal", false);
      runAx25(gpu::BitStream::TRANSITION, "transition", true);
      testAsk();
      testReconfig();
    }
  } catch (std::exception &e) { std::printf("FAIL: exception: %s\n", e.what()); return 2; }
  std::printf("%s (%d failures)\n", failures ? "FAILED" : "OK", failures);
  return failures ? 1 : 0;
}
