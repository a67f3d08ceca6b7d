// cut.cc — cuts the g18_* fixtures of the symbol path (FSKDetector, ASKDetector<int16_t>, BitStream) from the UNMODIFIED
// reference nodes, and times them on one core. TEST INFRASTRUCTURE: our own driver; it only includes the reference's
// headers at build time and links its objects where they lie (tools/golden_fsk/Makefile builds outside the tree).
//
//   cut golden <outdir>      write g18_*.bin + <outdir>/manifest_fsk.json
//   cut bench                time FSKDetector + BitStream over 1024 rows x 8192 samples (L = 18 and L = 242), JSON on stdout
//
// Inputs are synthesised here from a fixed-seed LCG: AFSK audio (phase-continuous tones keyed by random bits, noise added),
// stretches of exact silence, full-scale samples, and an FM-demodulated-looking +/- step signal for the ASK path.
#include "node.hh"
#include "fsk.hh"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <sstream>
#include <string>
#include <vector>

using namespace sdr;

static uint32_t g_lcg = 0x18f5c0deu;
static uint32_t lcg() { g_lcg = g_lcg * 1664525u + 1013904223u; return g_lcg >> 8; }
static double uni() { return (double)lcg() / 16777216.0 * 2.0 - 1.0; }

template <class T>
class Capture : public Sink<T> {
public:
  std::vector<T> data;
  std::vector<int32_t> lens;
  virtual void config(const Config &) {}
  virtual void process(const Buffer<T> &b, bool) {
    lens.push_back((int32_t)b.size());
    for (size_t i = 0; i < b.size(); i++) data.push_back(b[i]);
  }
};

template <class T>
class Feeder : public Source {
public:
  void configure(double Fs, size_t maxlen) { this->setConfig(Config(Config::typeId<T>(), Fs, maxlen, 1)); }
  void feed(T *p, size_t n) { Buffer<T> view(p, n); this->send(view, false); }
};

class FSKProbe : public FSKDetector {
public:
  FSKProbe(float baud, float fm, float fs) : FSKDetector(baud, fm, fs) {}
  std::vector<float> lut(bool mark) const {
    std::vector<float> v;
    for (size_t i = 0; i < _corrLen; i++) {
      const std::complex<float> c = mark ? _markLUT[i] : _spaceLUT[i];
      v.push_back(c.real()); v.push_back(c.imag());
    }
    return v;
  }
  size_t corrLen() const { return _corrLen; }
};

static std::vector<int16_t> afsk(double Fs, double baud, double fmark, double fspace, size_t n, double amp, double noise) {
  std::vector<int16_t> x(n);
  double phi = 0, bitpos = 0;
  int bit = 1;
  for (size_t i = 0; i < n; i++) {
    bitpos += baud / Fs;
    if (bitpos >= 1) { bitpos -= 1; if (lcg() & 1) bit ^= 1; }
    phi += 2 * M_PI * (bit ? fmark : fspace) / Fs;
    double v = amp * std::sin(phi) + noise * uni();
    x[i] = (int16_t)std::max(-32768.0, std::min(32767.0, std::floor(v + 0.5)));
  }
  return x;
}
static void silence(std::vector<int16_t> &x, size_t from, size_t len) { for (size_t i = from; i < from + len && i < x.size(); i++) x[i] = 0; }
static void fullscale(std::vector<int16_t> &x, size_t from, size_t len) {
  for (size_t i = from; i < from + len && i < x.size(); i++) x[i] = (lcg() & 1) ? 32767 : -32768;
}
static std::vector<int16_t> steps(double Fs, double baud, size_t n) {   // decaying +/- steps, as FM-demodulated FSK looks
  std::vector<int16_t> x(n);
  double level = 0, target = 6000, bitpos = 0;
  for (size_t i = 0; i < n; i++) {
    bitpos += baud / Fs;
    if (bitpos >= 1) { bitpos -= 1; if (lcg() & 1) target = -target; }
    level += 0.25 * (target - level);
    x[i] = (int16_t)std::floor(level + 900 * uni() + 0.5);
  }
  return x;
}

static std::string g_out;
static std::ostringstream g_manifest;
static bool g_first = true;
template <class T>
static void dump(const std::string &name, const char *dtype, const std::vector<T> &v, const std::string &extra = "") {
  const std::string path = g_out + "/" + name + ".bin";
  FILE *f = fopen(path.c_str(), "wb");
  if (!f) { perror(path.c_str()); exit(2); }
  if (v.size()) fwrite(&v[0], sizeof(T), v.size(), f);
  fclose(f);
  if (!g_first) g_manifest << ",\n";
  g_first = false;
  g_manifest << "  \"" << name << "\": {\"file\": \"" << name << ".bin\", \"dtype\": \"" << dtype << "\", \"count\": " << v.size();
  if (!extra.empty()) g_manifest << ", " << extra;
  g_manifest << "}";
}
static std::string lensJson(const std::vector<size_t> &lens) {
  std::ostringstream s; s << "[";
  for (size_t i = 0; i < lens.size(); i++) s << (i ? ", " : "") << lens[i];
  s << "]";
  return s.str();
}

// one stream through detector -> BitStream(mode) for both modes, in ragged buffers; reconf_at >= 0: the source's Config
// changes before that buffer (another buffer size), which re-runs config() down the chain
static void cutFsk(const std::string &name, double Fs, float baud, float fm, float fs, std::vector<int16_t> x,
                   const std::vector<size_t> &lens, int reconf_at = -1) {
  std::ostringstream par;
  par.precision(17);
  par << "\"Fs\": " << Fs << ", \"baud\": " << (double)baud << ", \"Fmark\": " << (double)fm << ", \"Fspace\": " << (double)fs
      << ", \"lens\": " << lensJson(lens) << ", \"reconf_at\": " << reconf_at;
  for (int mode = 0; mode < 2; mode++) {
    Feeder<int16_t> src;
    FSKProbe det(baud, fm, fs);
    BitStream bits(baud, mode ? BitStream::TRANSITION : BitStream::NORMAL);
    Capture<uint8_t> sym, out;
    src.connect(&det, true); det.connect(&sym, true); det.connect(&bits, true); bits.connect(&out, true);
    src.configure(Fs, 8192);
    std::vector<int32_t> per_buffer;
    size_t off = 0;
    for (size_t b = 0; b < lens.size(); b++) {
      if ((int)b == reconf_at) src.configure(Fs, 4096);
      const size_t before = out.data.size();
      src.feed(x.data() + off, lens[b]);
      off += lens[b];
      per_buffer.push_back((int32_t)(out.data.size() - before));
    }
    if (mode == 0) {
      std::ostringstream p2; p2 << par.str() << ", \"corr_len\": " << det.corrLen();
      dump(name + "_x", "i16", x, p2.str());
      dump(name + "_lut_mark", "cf32", det.lut(true), p2.str());
      dump(name + "_lut_space", "cf32", det.lut(false), p2.str());
      dump(name + "_sym", "u8", sym.data, p2.str());
    }
    const std::string tag = mode ? "_bits_transition" : "_bits_normal";
    dump(name + tag, "u8", out.data, par.str());
    dump(name + tag + "_counts", "i32", per_buffer, par.str());
  }
}

static void cutAsk(const std::string &name, double Fs, float baud, std::vector<int16_t> x, const std::vector<size_t> &lens) {
  std::ostringstream par;
  par.precision(17);
  par << "\"Fs\": " << Fs << ", \"baud\": " << (double)baud << ", \"lens\": " << lensJson(lens);
  dump(name + "_x", "i16", x, par.str());
  for (int inv = 0; inv < 2; inv++) {
    Feeder<int16_t> src;
    ASKDetector<int16_t> det(inv != 0);
    BitStream bits(baud, BitStream::NORMAL);
    Capture<uint8_t> sym, out;
    src.connect(&det, true); det.connect(&sym, true); det.connect(&bits, true); bits.connect(&out, true);
    src.configure(Fs, 8192);
    std::vector<int32_t> per_buffer;
    size_t off = 0;
    for (size_t b = 0; b < lens.size(); b++) {
      const size_t before = out.data.size();
      src.feed(x.data() + off, lens[b]);
      off += lens[b];
      per_buffer.push_back((int32_t)(out.data.size() - before));
    }
    const std::string tag = inv ? "_inv1" : "_inv0";
    dump(name + tag + "_sym", "u8", sym.data, par.str());
    dump(name + tag + "_bits_normal", "u8", out.data, par.str());
    dump(name + tag + "_bits_normal_counts", "i32", per_buffer, par.str());
  }
}

static int golden(const std::string &outdir) {
  g_out = outdir;
  const double Fs = 22050.0;
  {   // AX.25: 1200 baud, 1200 / 2200 Hz, L = 18; ragged buffers, an empty one included
    std::vector<size_t> lens = {4096, 1000, 1, 17, 3078, 0, 2048};
    std::vector<int16_t> x = afsk(Fs, 1200, 1200, 2200, 10240, 12000, 2500);
    silence(x, 2500, 700); fullscale(x, 5200, 300); silence(x, 9000, 40);
    cutFsk("g18_ax25", Fs, 1200.f, 1200.f, 2200.f, x, lens);
  }
  {   // RTTY: 90.90 baud, 930 / 1100 Hz, L = 242
    std::vector<size_t> lens = {8192, 5000, 241, 242, 243, 2466, 8192};
    std::vector<int16_t> x = afsk(Fs, 90.90, 930, 1100, 24576, 9000, 3000);
    silence(x, 6000, 1500); fullscale(x, 15000, 500);
    cutFsk("g18_rtty", Fs, 90.90f, 930.f, 1100.f, x, lens);
  }
  {   // a Config change in mid-stream: both nodes start over (rings, LUT index, PLL)
    std::vector<size_t> lens = {3000, 1111, 2000, 2081};
    std::vector<int16_t> x = afsk(Fs, 1200, 1200, 2200, 8192, 15000, 1500);
    cutFsk("g18_reconf", Fs, 1200.f, 1200.f, 2200.f, x, lens, 2);
  }
  {   // POCSAG's front end: ASKDetector(invert) -> BitStream(1200, NORMAL)
    std::vector<size_t> lens = {4096, 1000, 1, 17, 3078, 0};
    std::vector<int16_t> x = steps(Fs, 1200, 8192);
    silence(x, 3000, 200);
    cutAsk("g18_ask", Fs, 1200.f, x, lens);
  }
  FILE *f = fopen((outdir + "/manifest_fsk.json").c_str(), "w");
  if (!f) { perror("manifest_fsk.json"); return 2; }
  fprintf(f, "{\n%s\n}\n", g_manifest.str().c_str());
  fclose(f);
  return 0;
}

// FSKDetector -> BitStream on one core: `rows` independent streams of n samples each, one node pair per stream as a
// receiver bank would run them; warm-up, then `reps` timed passes; the median and the spread are reported.
static void benchOne(const char *name, double Fs, float baud, float fm, float fs, size_t rows, size_t n, int reps) {
  std::vector<int16_t> x = afsk(Fs, baud, fm, fs, n, 12000, 2500);
  std::vector<double> ms;
  for (int r = -1; r < reps; r++) {
    Feeder<int16_t> src;
    FSKDetector det(baud, fm, fs);
    BitStream bits(baud, BitStream::TRANSITION);
    Capture<uint8_t> out;
    src.connect(&det, true); det.connect(&bits, true); bits.connect(&out, true);
    src.configure(Fs, n);
    const size_t pass = r < 0 ? 8 : rows;
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    for (size_t c = 0; c < pass; c++) { out.data.clear(); out.lens.clear(); src.feed(x.data(), n); }
    const double dt = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (r >= 0) ms.push_back(dt);
  }
  std::sort(ms.begin(), ms.end());
  printf("  \"%s\": {\"rows\": %zu, \"n\": %zu, \"reps\": %d, \"cpu_reference_ms\": %.3f, \"min_ms\": %.3f, \"max_ms\": %.3f}", name, rows, n,
         reps, ms[ms.size() / 2], ms.front(), ms.back());
}

int main(int argc, char **argv) {
  if (argc >= 3 && std::string(argv[1]) == "golden") return golden(argv[2]);
  if (argc >= 2 && std::string(argv[1]) == "bench") {
    printf("{\n");
    benchOne("ax25_L18", 22050.0, 1200.f, 1200.f, 2200.f, 1024, 8192, 5);
    printf(",\n");
    benchOne("rtty_L242", 22050.0, 90.90f, 930.f, 1100.f, 1024, 8192, 3);
    printf("\n}\n");
    return 0;
  }
  fprintf(stderr, "usage: cut golden <outdir> | cut bench\n");
  return 1;
}
