// cut.cc — cuts the g22_inpol_* fixtures from the UNMODIFIED reference InpolSubSampler<iScalar, oScalar> (src/subsample.hh,
// src/interpolate.hh), and times the node on one core. TEST INFRASTRUCTURE: our own driver; it only includes the reference's
// headers at build time and links its objects where they lie (tools/golden_resample/Makefile builds outside the tree).
//
//   cut golden <outdir>      write g22_inpol_*.bin + <outdir>/manifest_resample.json
//   cut bench                time the node over 1024 rows x 8192 samples per type and frac, JSON on stdout
//
// The node is configured with a real sample rate (8000): InpolSubSampler::config sizes its output buffer as
// ceil(bufferSize * sampleRate / frac), which at a sample rate near 1 is too small for a call and is overrun.
// Inputs are synthesised here: two tones and noise from a fixed-seed LCG; the int16 inputs hold a full-scale stretch.
#include "node.hh"
#include "subsample.hh"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

using namespace sdr;

static uint32_t g_lcg = 0x22a51e57u;
static uint32_t lcg() { g_lcg = g_lcg * 1664525u + 1013904223u; return g_lcg >> 8; }
static double uni() { return (double)lcg() / 16777216.0 * 2.0 - 1.0; }

template <class T>
class Capture : public Sink<T> {
public:
  std::vector<T> data;
  virtual void config(const Config &) {}
  virtual void process(const Buffer<T> &b, bool) {
    for (size_t i = 0; i < b.size(); i++) data.push_back(b[i]);
  }
};

template <class T>
class Feeder : public Source {
public:
  void configure(double Fs, size_t maxlen) { this->setConfig(Config(Config::typeId<T>(), Fs, maxlen, 1)); }
  void feed(T *p, size_t n) { Buffer<T> view(p, n); this->send(view, false); }
};

template <class I, class O>
class Probe : public InpolSubSampler<I, O> {
public:
  Probe(float frac) : InpolSubSampler<I, O>(frac) {}
  float mu() const { return this->_mu; }
  O line(size_t k) const { return this->_dl[this->_dl_idx + k]; }   // oldest first
};

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

static const double FS = 8000.0;

// ---- inputs --------------------------------------------------------------------------------------------------------------------
static double tone(size_t i, double phase) {
  return 0.45 * std::sin(2 * M_PI * 440.0 * (double)i / FS + phase) + 0.25 * std::sin(2 * M_PI * 1730.0 * (double)i / FS + 2 * phase) + 0.02 * uni();
}
static int16_t to_i16(double v) { return (int16_t)std::max(-32768.0, std::min(32767.0, std::floor(v * 32767.0 + 0.5))); }
// the full-scale stretch of the int16 inputs: a step up to 32767 and a step down to -32768
static bool full_scale(size_t i, int16_t &v) {
  if (i >= 600 && i < 700) { v = 32767; return true; }
  if (i >= 700 && i < 800) { v = -32768; return true; }
  return false;
}

template <class T> static T sample(size_t i);
template <> float sample<float>(size_t i) { return (float)tone(i, 0.3); }
template <> std::complex<float> sample<std::complex<float> >(size_t i) { return std::complex<float>((float)tone(i, 0.3), (float)tone(i, 1.9)); }
template <> int16_t sample<int16_t>(size_t i) { int16_t v; if (full_scale(i, v)) return v; return to_i16(tone(i, 0.7)); }
template <> std::complex<int16_t> sample<std::complex<int16_t> >(size_t i) {
  int16_t v;
  if (full_scale(i, v)) return std::complex<int16_t>(v, (int16_t)(i < 650 || i >= 750 ? v : -v - 1));
  return std::complex<int16_t>(to_i16(tone(i, 0.7)), to_i16(tone(i, 2.4)));
}

static std::string g_out;
static std::ostringstream g_manifest;

template <class T>
static void writeBin(const std::string &file, const std::vector<T> &v) {
  const std::string path = g_out + "/" + file;
  FILE *f = fopen(path.c_str(), "wb");
  if (!f) { perror(path.c_str()); exit(2); }
  if (v.size()) fwrite(&v[0], sizeof(T), v.size(), f);
  fclose(f);
}

template <class I, class O>
static void cut(const std::string &dtype, const std::string &tag, float frac, std::vector<I> &x, const std::vector<size_t> &lens) {
  const std::string name = "g22_inpol_" + dtype + "_" + tag;
  Feeder<I> src;
  Probe<I, O> node(frac);
  Capture<O> out;
  src.connect(&node, true); node.connect(&out, true);
  size_t longest = 0;
  for (size_t b = 0; b < lens.size(); b++) longest = std::max(longest, lens[b]);
  src.configure(FS, longest);
  std::ostringstream mu, counts;
  std::vector<O> lines;
  size_t off = 0, before = 0;
  for (size_t b = 0; b < lens.size(); b++) {
    src.feed(x.data() + off, lens[b]);
    off += lens[b];
    counts << (b ? ", " : "") << out.data.size() - before;
    before = out.data.size();
    mu << (b ? ", " : "") << bits(node.mu());
    for (size_t k = 0; k < 8; k++) lines.push_back(node.line(k));
  }
  writeBin(name + "_y.bin", out.data);
  writeBin(name + "_lines.bin", lines);
  g_manifest.precision(9);
  g_manifest << "  \"" << name << "\": {\"dtype\": \"" << dtype << "\", \"count\": " << off << ", \"outputs\": " << out.data.size() << ", \"x\": \"g22_inpol_"
             << dtype << "_x.bin\", \"y\": \"" << name << "_y.bin\", \"lines\": \"" << name << "_lines.bin\", \"Fs\": " << FS << ", \"frac\": " << frac
             << ", \"frac_bits\": " << bits(frac) << ", \"lens\": [";
  for (size_t i = 0; i < lens.size(); i++) g_manifest << (i ? ", " : "") << lens[i];
  g_manifest << "], \"counts\": [" << counts.str() << "], \"mu_bits\": [" << mu.str() << "]},\n";
  fprintf(stderr, "%s: %zu samples -> %zu outputs\n", name.c_str(), off, out.data.size());
}

static const float FRACS[] = {0.5f, 1.378125f, 2.0f, 7.9f};
static const char *TAGS[] = {"0p5", "1p378125", "2", "7p9"};

template <class I, class O>
static void cutType(const std::string &dtype, const std::vector<size_t> &lens) {
  size_t n = 0;
  for (size_t i = 0; i < lens.size(); i++) n += lens[i];
  std::vector<I> x(n);
  for (size_t i = 0; i < n; i++) x[i] = sample<I>(i);
  writeBin("g22_inpol_" + dtype + "_x.bin", x);
  for (int k = 0; k < 4; k++) cut<I, O>(dtype, TAGS[k], FRACS[k], x, lens);
}

static int golden(const std::string &outdir) {
  g_out = outdir;
  const std::vector<size_t> lens = {5, 5, 1, 256, 257, 0, 773, 300, 1000, 999, 400};   // 3996
  cutType<float, float>("f32", lens);
  cutType<std::complex<float>, std::complex<float> >("cf32", lens);
  cutType<int16_t, int16_t>("i16", lens);
  cutType<std::complex<int16_t>, std::complex<float> >("cs16_cf32", lens);
  FILE *f = fopen((outdir + "/manifest_resample.json").c_str(), "w");
  if (!f) { perror("manifest_resample.json"); return 2; }
  fprintf(f, "{\n%s  \"table\": \"g21_psk31_table.bin\"\n}\n", g_manifest.str().c_str());
  fclose(f);
  return 0;
}

// `rows` independent streams of n samples each on one core, one node per stream as a bank would run them, in calls of 1024;
// warm-up, then `reps` timed passes; the median and the spread are reported.
template <class I, class O>
static void benchOne(const std::string &name, float frac, size_t rows, size_t n, int reps) {
  std::vector<I> x(n);
  for (size_t i = 0; i < n; i++) x[i] = sample<I>(i + 1000);
  std::vector<double> ms;
  size_t outputs = 0;
  for (int r = -1; r < reps; r++) {
    const size_t pass = r < 0 ? 8 : rows;
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    for (size_t c = 0; c < pass; c++) {
      Feeder<I> src;
      InpolSubSampler<I, O> node(frac);
      Capture<O> out;
      src.connect(&node, true); node.connect(&out, true);
      src.configure(FS, 1024);
      out.data.reserve((size_t)((double)n / frac) + 16);
      for (size_t off = 0; off < n; off += 1024) src.feed(x.data() + off, std::min((size_t)1024, n - off));
      outputs = out.data.size();
    }
    const double dt = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (r >= 0) ms.push_back(dt);
  }
  std::sort(ms.begin(), ms.end());
  printf("  \"%s\": {\"rows\": %zu, \"n\": %zu, \"frac\": %.9g, \"outputs_per_row\": %zu, \"reps\": %d, \"cpu_reference_ms\": %.3f, \"min_ms\": %.3f, "
         "\"max_ms\": %.3f}", name.c_str(), rows, n, (double)frac, outputs, reps, ms[ms.size() / 2], ms.front(), ms.back());
}

template <class I, class O>
static void benchType(const std::string &dtype, bool first) {
  const float fracs[] = {0.5f, 1.378125f, 7.9f};
  const char *tags[] = {"0p5", "1p378125", "7p9"};
  for (int k = 0; k < 3; k++) {
    if (!first || k) printf(",\n");
    benchOne<I, O>("inpol_" + dtype + "_" + tags[k], fracs[k], 1024, 8192, 3);
  }
}

int main(int argc, char **argv) {
  if (argc >= 3 && std::string(argv[1]) == "golden") return golden(argv[2]);
  if (argc >= 2 && std::string(argv[1]) == "bench") {
    printf("{\n");
    benchType<float, float>("f32", true);
    benchType<std::complex<float>, std::complex<float> >("cf32", false);
    benchType<int16_t, int16_t>("i16", false);
    benchType<std::complex<int16_t>, std::complex<float> >("cs16_cf32", false);
    printf("\n}\n");
    return 0;
  }
  fprintf(stderr, "usage: cut golden <outdir> | cut bench\n");
  return 1;
}
