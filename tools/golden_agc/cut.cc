// cut.cc — cuts the g20_agc_* fixtures from the UNMODIFIED reference AGC<int16_t> / AGC<float> (src/utils.hh), and times the
// node on one core. TEST INFRASTRUCTURE: our own driver; it only includes the reference's headers at build time and links its
// objects where they lie (tools/golden_agc/Makefile builds outside the tree).
//
//   cut golden <outdir>      write g20_agc_*.bin + <outdir>/manifest_agc.json
//   cut bench                time AGC<int16_t> and AGC<float> over 1024 rows x 8192 samples, JSON on stdout
//
// Inputs are synthesised here from a fixed-seed LCG: tones with noise, stretches of exact zeros, full-scale bursts, a quiet
// tail with full-scale spikes in it (a high crest factor: hundreds of int16 products wrap). AGC::process sends its WHOLE output buffer whatever the input's length; the capture keeps the first n samples of each
// buffer it is sent (n: the length of the buffer fed), which is what the GPU node delivers.
#include "node.hh"
#include "utils.hh"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

using namespace sdr;

static uint32_t g_lcg = 0x20a6c0deu;
static uint32_t lcg() { g_lcg = g_lcg * 1664525u + 1013904223u; return g_lcg >> 8; }
static double uni() { return (double)lcg() / 16777216.0 * 2.0 - 1.0; }

template <class T>
class Capture : public Sink<T> {
public:
  std::vector<T> data;
  size_t want = 0;
  virtual void config(const Config &) {}
  virtual void process(const Buffer<T> &b, bool) {
    for (size_t i = 0; i < want && i < b.size(); i++) data.push_back(b[i]);
  }
};

template <class T>
class Feeder : public Source {
public:
  void configure(double Fs, size_t maxlen) { this->setConfig(Config(Config::typeId<T>(), Fs, maxlen, 1)); }
  void feed(T *p, size_t n) { Buffer<T> view(p, n); this->send(view, false); }
};

template <class T>
class Probe : public AGC<T> {
public:
  Probe(double tau, double target) : AGC<T>(tau, target) {}
  float lambda() const { return this->_lambda; }
  float sd() const { return this->_sd; }
  float target() const { return this->_target; }
};

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

// what happens before buffer `at`: 'e' enable(value != 0), 'g' setGain(value)
struct Op { int at; char what; float value; };

template <class T> static T sample(double v);
template <> int16_t sample<int16_t>(double v) { return (int16_t)std::max(-32768.0, std::min(32767.0, std::floor(v * 32767.0 + 0.5))); }
template <> float sample<float>(double v) { return (float)v; }

// tones with noise at amplitude amp (of full scale), then the edits below
template <class T>
static std::vector<T> tones(double Fs, size_t n, double amp, double noise) {
  std::vector<T> x(n);
  for (size_t i = 0; i < n; i++) {
    const double t = (double)i / Fs;
    x[i] = sample<T>(amp * (0.6 * std::sin(2 * M_PI * 440.0 * t) + 0.4 * std::sin(2 * M_PI * 1333.0 * t + 0.7)) + noise * uni());
  }
  return x;
}
template <class T> static void zeros(std::vector<T> &x, size_t from, size_t len) { for (size_t i = from; i < from + len && i < x.size(); i++) x[i] = T(0); }
template <class T> static void burst(std::vector<T> &x, size_t from, size_t len) {
  for (size_t i = from; i < from + len && i < x.size(); i++) x[i] = (lcg() & 1) ? sample<T>(1.0) : (sizeof(T) == 2 ? T(-32768) : T(-1));
}
template <class T> static void spikes(std::vector<T> &x, size_t from, size_t every) {   // a high crest factor: int16 products wrap
  for (size_t i = from; i < x.size(); i += every) x[i] = (lcg() & 1) ? sample<T>(1.0) : (sizeof(T) == 2 ? T(-32768) : T(-1));
}
template <class T> static void quiet(std::vector<T> &x, size_t from, double factor) {
  for (size_t i = from; i < x.size(); i++) x[i] = sample<T>((double)x[i] / (sizeof(T) == 2 ? 32767.0 : 1.0) * factor);
}

static std::string g_out;
static std::ostringstream g_manifest;
static bool g_first = true;

template <class T>
static void writeBin(const std::string &file, const std::vector<T> &v) {
  const std::string path = g_out + "/" + file;
  FILE *f = fopen(path.c_str(), "wb");
  if (!f) { perror(path.c_str()); exit(2); }
  if (v.size()) fwrite(&v[0], sizeof(T), v.size(), f);
  fclose(f);
}

template <class T>
static void cut(const std::string &name, double Fs, double tau, double target, std::vector<T> x, const std::vector<size_t> &lens,
                const std::vector<Op> &ops = std::vector<Op>()) {
  Feeder<T> src;
  Probe<T> agc(tau, target);
  Capture<T> out;
  src.connect(&agc, true); agc.connect(&out, true);
  src.configure(Fs, 8192);
  std::ostringstream state;
  size_t off = 0;
  for (size_t b = 0; b < lens.size(); b++) {
    for (size_t k = 0; k < ops.size(); k++)
      if (ops[k].at == (int)b) { if (ops[k].what == 'e') agc.enable(ops[k].value != 0); else agc.setGain(ops[k].value); }
    out.want = lens[b];
    src.feed(x.data() + off, lens[b]);
    off += lens[b];
    state << (b ? ", " : "") << "[" << bits(agc.gain()) << ", " << bits(agc.sd()) << ", " << (agc.enabled() ? 1 : 0) << "]";
  }
  if (off != x.size() || out.data.size() != x.size()) { fprintf(stderr, "%s: %zu fed, %zu captured of %zu\n", name.c_str(), off, out.data.size(), x.size()); exit(3); }
  writeBin(name + "_x.bin", x);
  writeBin(name + "_y.bin", out.data);
  if (!g_first) g_manifest << ",\n";
  g_first = false;
  g_manifest.precision(17);
  g_manifest << "  \"" << name << "\": {\"dtype\": \"" << (sizeof(T) == 2 ? "i16" : "f32") << "\", \"count\": " << x.size() << ", \"x\": \"" << name
             << "_x.bin\", \"y\": \"" << name << "_y.bin\", \"Fs\": " << Fs << ", \"tau\": " << tau << ", \"target\": " << target
             << ", \"lambda_bits\": " << bits(agc.lambda()) << ", \"target_bits\": " << bits(agc.target()) << ", \"lens\": [";
  for (size_t i = 0; i < lens.size(); i++) g_manifest << (i ? ", " : "") << lens[i];
  g_manifest << "], \"ops\": [";
  for (size_t k = 0; k < ops.size(); k++)
    g_manifest << (k ? ", " : "") << "{\"at\": " << ops[k].at << ", \"what\": \"" << (ops[k].what == 'e' ? "enable" : "gain") << "\", \"value_bits\": "
               << bits(ops[k].value) << "}";
  g_manifest << "], \"state_bits\": [" << state.str() << "]}";
}

template <class T>
static void cutType(const std::string &tag) {
  const std::vector<size_t> ragged = {4096, 1000, 1, 17, 3078, 0, 2048};   // 10240
  {   // the default target: tones, 1500 zeros, a full-scale burst right behind them, a quiet tail with full-scale spikes in it
    std::vector<T> x = tones<T>(22050.0, 10240, 0.3, 0.05);
    zeros(x, 2500, 1500); burst(x, 4000, 300); zeros(x, 6000, 500); burst(x, 6500, 40); quiet(x, 8200, 0.01); spikes(x, 8300, 16);
    cut<T>("g20_agc_" + tag + "_default", 22050.0, 0.02, 0.0, x, ragged);
  }
  {   // an explicit target at another sample rate and a fast time constant: 2000 zeros, bursts
    const std::vector<size_t> lens = {2048, 0, 3000, 17, 1, 5174};   // 10240
    std::vector<T> x = tones<T>(48000.0, 10240, 0.1, 0.02);
    zeros(x, 1000, 2000); burst(x, 3000, 200); burst(x, 7000, 3); quiet(x, 9000, 0.003);
    cut<T>("g20_agc_" + tag + "_target", 48000.0, 0.002, sizeof(T) == 2 ? 9000.0 : 0.25, x, lens);
  }
  {   // the setters between buffers: held gain, pass-through, a set gain, enabled again
    const std::vector<size_t> lens = {1024, 700, 1, 1000, 323, 1024, 0, 1000, 1072};   // 6144
    std::vector<T> x = tones<T>(22050.0, 6144, 0.2, 0.04);
    zeros(x, 1500, 600); burst(x, 2100, 100); burst(x, 5000, 50);
    const std::vector<Op> ops = {{1, 'e', 0.f}, {3, 'g', 0.f}, {4, 'g', 2.5f}, {5, 'e', 1.f}, {7, 'e', 0.f}, {7, 'g', 0.f}, {8, 'e', 1.f}};
    cut<T>("g20_agc_" + tag + "_ops", 22050.0, 0.01, 0.0, x, lens, ops);
  }
  {   // silence until sd is denormal and the gain +inf: lambda = exp(-1/8); one non-zero sample inside the zeros
    const std::vector<size_t> lens = {512, 1000, 488, 48};   // 2048
    std::vector<T> x = tones<T>(8000.0, 2048, 0.25, 0.03);
    zeros(x, 300, 1400); x[350] = sample<T>(0.01);   // (buffer 1 ends 1161 zeros behind it: sd denormal, gain +inf)
    cut<T>("g20_agc_" + tag + "_silence", 8000.0, 0.001, 0.0, x, lens);
  }
}

static int golden(const std::string &outdir) {
  g_out = outdir;
  cutType<int16_t>("i16");
  cutType<float>("f32");
  FILE *f = fopen((outdir + "/manifest_agc.json").c_str(), "w");
  if (!f) { perror("manifest_agc.json"); return 2; }
  fprintf(f, "{\n%s\n}\n", g_manifest.str().c_str());
  fclose(f);
  return 0;
}

// `rows` independent streams of n samples each on one core, one node per stream as a bank would run them; warm-up, then
// `reps` timed passes; the median and the spread are reported.
template <class T>
static void benchOne(const char *name, size_t rows, size_t n, int reps) {
  std::vector<T> x = tones<T>(22050.0, n, 0.3, 0.05);
  std::vector<double> ms;
  for (int r = -1; r < reps; r++) {
    Feeder<T> src;
    AGC<T> agc(0.1, 0.0);
    Capture<T> out;
    src.connect(&agc, true); agc.connect(&out, true);
    src.configure(22050.0, n);
    out.want = 1;
    const size_t pass = r < 0 ? 8 : rows;
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    for (size_t c = 0; c < pass; c++) { out.data.clear(); src.feed(x.data(), n); }
    const double dt = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (r >= 0) ms.push_back(dt);
  }
  std::sort(ms.begin(), ms.end());
  printf("  \"%s\": {\"rows\": %zu, \"n\": %zu, \"reps\": %d, \"cpu_reference_ms\": %.3f, \"min_ms\": %.3f, \"max_ms\": %.3f}", name, rows, n, reps,
         ms[ms.size() / 2], ms.front(), ms.back());
}

int main(int argc, char **argv) {
  if (argc >= 3 && std::string(argv[1]) == "golden") return golden(argv[2]);
  if (argc >= 2 && std::string(argv[1]) == "bench") {
    printf("{\n");
    benchOne<int16_t>("agc_i16", 1024, 8192, 5);
    printf(",\n");
    benchOne<float>("agc_f32", 1024, 8192, 5);
    printf("\n}\n");
    return 0;
  }
  fprintf(stderr, "usage: cut golden <outdir> | cut bench\n");
  return 1;
}
