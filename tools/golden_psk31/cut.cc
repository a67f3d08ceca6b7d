// cut.cc — cuts the g21_psk31_* / g21_varicode_* fixtures from the UNMODIFIED reference BPSK31<int16_t> / BPSK31<float> and
// Varicode (src/psk31.hh, src/psk31.cc), and times the demodulator on one core. TEST INFRASTRUCTURE: our own driver; it only
// includes the reference's headers at build time and links its objects where they lie (tools/golden_psk31/Makefile builds
// outside the tree).
//
//   cut golden <outdir>      write g21_*.bin + <outdir>/manifest_psk31.json
//   cut bench                time BPSK31<int16_t> and BPSK31<float> over 1024 rows x 8192 samples, JSON on stdout
//
// Inputs are synthesised here: a PSK31 modulator (31.25 baud, a reversal per 0 bit with a cosine-shaped envelope, a carrier
// offset, noise from a fixed-seed LCG) fed by a Varicode encoder for lower-case text. Every call is at most one second long:
// BPSK31::config sizes the node's output buffer for one second and a longer call overruns it.
#include "node.hh"
#include "psk31.hh"

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

static uint32_t g_lcg = 0x21b5c31fu;
static uint32_t lcg() { g_lcg = g_lcg * 1664525u + 1013904223u; return g_lcg >> 8; }
static double uni() { return (double)lcg() / 16777216.0 * 2.0 - 1.0; }

class Capture : public Sink<uint8_t> {
public:
  std::vector<uint8_t> data;
  virtual void config(const Config &) {}
  virtual void process(const Buffer<uint8_t> &b, bool) {
    for (size_t i = 0; i < b.size(); i++) data.push_back(b[i]);
  }
};

template <class T>
class Feeder : public Source {
public:
  void configure(double Fs, size_t maxlen) { this->setConfig(Config(Config::typeId<T>(), Fs, maxlen, 1)); }
  void feed(T *p, size_t n) { Buffer<T> view(p, n); this->send(view, false); }
};

template <class T>
class Probe : public BPSK31<T> {
public:
  Probe(double dF) : BPSK31<T>(dF) {}
  float P() const { return this->_P; }
  float F() const { return this->_F; }
  float mu() const { return this->_mu; }
  float omega() const { return this->_omega; }
  float alpha() const { return this->_alpha; }
  float beta() const { return this->_beta; }
  float minOmega() const { return this->_min_omega; }
  float maxOmega() const { return this->_max_omega; }
  int histIdx() const { return (int)this->_hist_idx; }
  int last() const { return this->_last_constellation; }
};

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

// ---- Varicode encoder (lower-case letters and the space; codes of the published PSK31 table) ---------------------------------
static const char *letter_code(char ch) {
  static const char *lower[26] = {"1011", "1011111", "101111", "101101", "11", "111101", "1011011", "101011", "1101", "111101011", "10111111",
                                  "11011", "111011", "1111", "111", "111111", "110111111", "10101", "10111", "101", "110111", "1111011",
                                  "1101011", "11011111", "1011101", "111010101"};
  if (ch == ' ') return "1";
  if (ch >= 'a' && ch <= 'z') return lower[ch - 'a'];
  fprintf(stderr, "no code for '%c'\n", ch); exit(4);
}
// `idle` zero bits, the characters each followed by 00, then zeros up to `total` bits
static std::vector<uint8_t> encode(const std::string &text, size_t idle, size_t total) {
  std::vector<uint8_t> b(idle, 0);
  for (size_t i = 0; i < text.size(); i++) {
    for (const char *p = letter_code(text[i]); *p; p++) b.push_back(*p == '1');
    b.push_back(0); b.push_back(0);
  }
  while (b.size() < total) b.push_back(0);
  return b;
}

// ---- modulator ---------------------------------------------------------------------------------------------------------------
template <class T> static std::complex<T> sample(std::complex<double> v);
template <> std::complex<int16_t> sample<int16_t>(std::complex<double> v) {
  return std::complex<int16_t>((int16_t)std::max(-32768.0, std::min(32767.0, std::floor(v.real() * 32767.0 + 0.5))),
                               (int16_t)std::max(-32768.0, std::min(32767.0, std::floor(v.imag() * 32767.0 + 0.5))));
}
template <> std::complex<float> sample<float>(std::complex<double> v) { return std::complex<float>((float)v.real(), (float)v.imag()); }

struct Signal { double Fs, baud, offset_hz, phase, amp, noise; size_t zeros; };

template <class T>
static std::vector<std::complex<T> > modulate(const Signal &s, size_t n, const std::vector<uint8_t> &b) {
  std::vector<double> a(b.size() + 2);
  a[0] = 1.0;
  for (size_t k = 0; k < b.size(); k++) a[k + 1] = b[k] ? a[k] : -a[k];
  a[b.size() + 1] = a[b.size()];
  const double T_sym = s.Fs / s.baud;
  std::vector<std::complex<T> > x(n);
  for (size_t i = 0; i < n; i++) {
    if (i < s.zeros) { x[i] = std::complex<T>(0, 0); continue; }
    const double t = (double)(i - s.zeros) / T_sym;
    const size_t k = std::min((size_t)t, b.size());
    const double frac = t - (double)k;
    const double m = a[k] == a[k + 1] ? a[k] : a[k] * std::cos(M_PI * frac);
    const double ph = 2 * M_PI * s.offset_hz * (double)i / s.Fs + s.phase;
    x[i] = sample<T>(s.amp * m * std::complex<double>(std::cos(ph), std::sin(ph)) + s.noise * std::complex<double>(uni(), uni()));
  }
  return x;
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

template <class T>
static void cut(const std::string &name, const Signal &s, double dF, const std::string &text, const std::vector<size_t> &lens) {
  size_t n = 0;
  for (size_t i = 0; i < lens.size(); i++) n += lens[i];
  const std::vector<uint8_t> tx = encode(text, 24, (size_t)((double)n / (s.Fs / s.baud)) + 4);
  std::vector<std::complex<T> > x = modulate<T>(s, n, tx);

  Feeder<std::complex<T> > src;
  Probe<T> node(dF);
  Capture out;
  src.connect(&node, true); node.connect(&out, true);
  src.configure(s.Fs, (size_t)s.Fs);
  std::ostringstream state, counts;
  size_t off = 0, before = 0;
  for (size_t b = 0; b < lens.size(); b++) {
    if ((double)lens[b] > s.Fs) { fprintf(stderr, "%s: a call of %zu samples is longer than one second\n", name.c_str(), lens[b]); exit(3); }
    src.feed(x.data() + off, lens[b]);
    off += lens[b];
    counts << (b ? ", " : "") << out.data.size() - before;
    before = out.data.size();
    state << (b ? ", " : "") << "[" << bits(node.P()) << ", " << bits(node.F()) << ", " << bits(node.mu()) << ", " << bits(node.omega()) << ", "
          << node.histIdx() << ", " << node.last() << "]";
  }
  // for information: the same row one sample per call; a call that starts with mu <= 1 takes a sub-sample with that mu
  size_t row128 = 0, subs = 0;
  {
    Feeder<std::complex<T> > src1;
    Probe<T> one(dF);
    Capture out1;
    src1.connect(&one, true); one.connect(&out1, true);
    src1.configure(s.Fs, (size_t)s.Fs);
    for (size_t i = 0; i < n; i++) {
      const float mu = one.mu();
      if (!(mu > 1)) { subs++; if ((int)roundf(mu * 128) == 128) row128++; }
      src1.feed(x.data() + i, 1);
    }
    if (out1.data != out.data) { fprintf(stderr, "%s: the one-sample calls decode other bits\n", name.c_str()); exit(3); }
  }
  writeBin(name + "_x.bin", x);
  writeBin(name + "_bits.bin", out.data);
  g_manifest.precision(17);
  g_manifest << "  \"" << name << "\": {\"dtype\": \"" << (sizeof(T) == 2 ? "cs16" : "cf32") << "\", \"count\": " << n << ", \"x\": \"" << name
             << "_x.bin\", \"bits\": \"" << name << "_bits.bin\", \"Fs\": " << s.Fs << ", \"dF\": " << dF << ", \"baud\": " << s.baud
             << ", \"offset_hz\": " << s.offset_hz << ", \"text\": \"" << text << "\", \"alpha_bits\": " << bits(node.alpha())
             << ", \"beta_bits\": " << bits(node.beta()) << ", \"min_omega_bits\": " << bits(node.minOmega()) << ", \"max_omega_bits\": "
             << bits(node.maxOmega()) << ", \"sub_samples_first_of_sample\": " << subs << ", \"row128_sub_samples\": " << row128 << ", \"lens\": [";
  for (size_t i = 0; i < lens.size(); i++) g_manifest << (i ? ", " : "") << lens[i];
  g_manifest << "], \"counts\": [" << counts.str() << "], \"state_bits\": [" << state.str() << "]},\n";
  fprintf(stderr, "%s: %zu bits, %zu of %zu sub-samples on table row 128\n", name.c_str(), out.data.size(), row128, subs);
}

// every value 1 ... 4095 whose binary form holds no 00, each followed by 00; fed in ragged calls that end inside codes
static void cutVaricode() {
  std::vector<uint8_t> b;
  for (int v = 1; v < 4096; v++) {
    bool ok = true;
    int top = 11;
    while (!((v >> top) & 1)) top--;
    for (int k = top; k >= 1; k--) if (!((v >> k) & 1) && !((v >> (k - 1)) & 1)) ok = false;
    if (!ok) continue;
    for (int k = top; k >= 0; k--) b.push_back((v >> k) & 1);
    b.push_back(0); b.push_back(0);
  }
  Feeder<uint8_t> src;
  Varicode node;
  Capture out;
  src.connect(&node, true); node.connect(&out, true);
  src.configure(31.25, 18);
  // (Varicode's output buffer holds 18 characters: a call of at most 18 bits cannot overrun it)
  const size_t pattern[] = {18, 1, 7, 13, 2, 17, 5, 11, 3};
  std::ostringstream lens, counts;
  size_t off = 0, before = 0, k = 0;
  while (off < b.size()) {
    const size_t len = std::min(pattern[k % 9], b.size() - off);
    src.feed(b.data() + off, len);
    off += len;
    lens << (k ? ", " : "") << len;
    counts << (k ? ", " : "") << out.data.size() - before;
    before = out.data.size();
    k++;
  }
  writeBin("g21_varicode_bits.bin", b);
  writeBin("g21_varicode_text.bin", out.data);
  g_manifest << "  \"g21_varicode\": {\"bits\": \"g21_varicode_bits.bin\", \"text\": \"g21_varicode_text.bin\", \"count\": " << b.size()
             << ", \"chars\": " << out.data.size() << ", \"lens\": [" << lens.str() << "], \"counts\": [" << counts.str() << "]},\n";
}

static int golden(const std::string &outdir) {
  g_out = outdir;
  {   // the interpolation table as the running reference holds it
    std::vector<float> t(129 * 8);
    for (int r = 0; r < 129; r++) for (int k = 0; k < 8; k++) t[r * 8 + k] = interpolate_taps[r][k];
    writeBin("g21_psk31_table.bin", t);
  }
  {   // the C library's sincosf behind std::exp(complex<float>(0, P)): 4096 arguments of [-2 pi, 2 pi], as (P, sin, cos)
    std::vector<float> p(4096 * 3);
    for (int i = 0; i < 4096; i++) {
      const float P = i < 2 ? (i ? (float)(2 * M_PI) : (float)(-2 * M_PI)) : (float)(uni() * 2 * M_PI);
      const std::complex<float> f = std::exp(std::complex<float>(0, P));
      p[3 * i] = P; p[3 * i + 1] = f.imag(); p[3 * i + 2] = f.real();
    }
    writeBin("g21_psk31_sincosf.bin", p);
  }
  const std::vector<size_t> l8k = {8000, 5000, 1, 33, 999, 0, 7967, 2000};   // 24000
  const std::vector<size_t> l2k = {2000, 1500, 1, 33, 466, 0, 2000};         // 6000
  const Signal base8 = {8000.0, 31.25, 3.0, 0.4, 0.5, 0.01, 0};
  { Signal s = base8; s.offset_hz = 2.0; s.noise = 0.004; cut<int16_t>("g21_psk31_cs16_8k", s, 0.1, "cq de gpu", l8k); }
  { Signal s = base8; s.offset_hz = -5.0; s.phase = 2.1; cut<float>("g21_psk31_cf32_8k", s, 0.1, "the quick", l8k); }
  { Signal s = base8; s.Fs = 2000.0; s.offset_hz = 1.0; s.phase = -1.0; cut<float>("g21_psk31_cf32_2k", s, 0.1, "psk", l2k); }
  { Signal s = base8; s.offset_hz = 6.0; cut<int16_t>("g21_psk31_cs16_clamp", s, 0.002, "clamp", l8k); }      // F rides its clamp
  { Signal s = base8; s.zeros = 2500; s.noise = 0.0; s.offset_hz = 1.5; cut<float>("g21_psk31_cf32_zeros", s, 0.1, "zero", l8k); }
  { Signal s = base8; s.baud = 31.25 * 1.0005; s.offset_hz = -2.0; cut<int16_t>("g21_psk31_cs16_baud", s, 0.1, "baud off", l8k); }
  cutVaricode();
  FILE *f = fopen((outdir + "/manifest_psk31.json").c_str(), "w");
  if (!f) { perror("manifest_psk31.json"); return 2; }
  fprintf(f, "{\n%s  \"table\": \"g21_psk31_table.bin\", \"sincosf\": \"g21_psk31_sincosf.bin\"\n}\n", g_manifest.str().c_str());
  fclose(f);
  return 0;
}

// `rows` independent streams of n samples each on one core, one node per stream as a bank would run them, in calls of at most
// one second; warm-up, then `reps` timed passes; the median and the spread are reported.
template <class T>
static void benchOne(const char *name, size_t rows, size_t n, int reps) {
  const Signal s = {8000.0, 31.25, 3.0, 0.4, 0.5, 0.01, 0};
  std::vector<std::complex<T> > x = modulate<T>(s, n, encode("bench", 8, n / 256 + 4));
  std::vector<double> ms;
  for (int r = -1; r < reps; r++) {
    const size_t pass = r < 0 ? 8 : rows;
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    for (size_t c = 0; c < pass; c++) {
      Feeder<std::complex<T> > src;
      BPSK31<T> node(0.1);
      Capture out;
      src.connect(&node, true); node.connect(&out, true);
      src.configure(8000.0, 8000);
      for (size_t off = 0; off < n; off += 4096) src.feed(x.data() + off, std::min((size_t)4096, n - off));
    }
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
    benchOne<int16_t>("psk31_cs16", 1024, 8192, 3);
    printf(",\n");
    benchOne<float>("psk31_cf32", 1024, 8192, 3);
    printf("\n}\n");
    return 0;
  }
  fprintf(stderr, "usage: cut golden <outdir> | cut bench\n");
  return 1;
}
