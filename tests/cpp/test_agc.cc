// test_agc.cc — sdr::gpu::AGC<int16_t>, gpu::AGC<float> and gpu::AGCBank (include/sdr/gpu/agc.hh) on the GPU against the
// g20_agc_* fixtures of the compiled reference. Every stream runs through Source -> gpu::AGC -> Sink in its recorded buffers,
// with the recorded enable() / setGain() calls in front of them; after every buffer the output, gain() and level() must be the
// reference's bits (float outputs: except where both sides are NaN). Then the first 1024 samples of every stream of a type are
// the device rows of one AGCBank::processDev call.
//   test_agc <cases.txt> <golden dir> <tau.txt>
// tau.txt, one line per type: name dtype Fs tau target tau2 n1 n2 gain1 sd1 gain2 sd2 expected.bin — setTau(tau2) between two
// buffers of n1 and n2 samples of the stream; the expectation is the restatement's (the reference's setTau changes the decay alone).
// cases.txt, one stream per line: name dtype Fs tau target count  nlens lens...  nops (at what value_bits)...  (gain_bits sd_bits) per buffer
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "sdr/gpu/agc.hh"

using namespace sdr;

struct Op { int at; int what; uint32_t bits; };   // what: 0 enable, 1 gain
struct Case {
  std::string name, dtype;
  double Fs, tau, target;
  size_t count;
  std::vector<size_t> lens;
  std::vector<Op> ops;
  std::vector<uint32_t> gain, sd;
};

static uint32_t bitsOf(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float floatOf(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static bool same(int16_t a, int16_t b) { return a == b; }
static bool same(float a, float b) { return (std::isnan(a) && std::isnan(b)) || bitsOf(a) == bitsOf(b); }

template <class T>
static std::vector<T> readBin(const std::string &path, size_t count) {
  std::vector<T> v(count);
  std::ifstream f(path.c_str(), std::ios::binary);
  f.read(reinterpret_cast<char *>(v.data()), count * sizeof(T));
  if ((size_t)f.gcount() != count * sizeof(T)) { fprintf(stderr, "%s: short file\n", path.c_str()); exit(2); }
  return v;
}

template <class T>
class Capture : public Sink<T> {
public:
  std::vector<T> data;
  virtual void config(const Config &) {}
  virtual void process(const Buffer<T> &b, bool) {
    data.clear();
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
static int runNode(const Case &k, const std::string &dir, size_t &samples) {
  std::vector<T> x = readBin<T>(dir + "/" + k.name + "_x.bin", k.count), y = readBin<T>(dir + "/" + k.name + "_y.bin", k.count);
  Feeder<T> src;
  gpu::AGC<T> agc(k.tau, k.target);
  Capture<T> out;
  src.connect(&agc, true); agc.connect(&out, true);
  src.configure(k.Fs, 8192);
  int failures = 0;
  size_t off = 0;
  for (size_t b = 0; b < k.lens.size(); b++) {
    for (size_t i = 0; i < k.ops.size(); i++)
      if (k.ops[i].at == (int)b) { if (k.ops[i].what == 0) agc.enable(floatOf(k.ops[i].bits) != 0); else agc.setGain(floatOf(k.ops[i].bits)); }
    const size_t n = k.lens[b];
    out.data.clear();
    src.feed(x.data() + off, n);
    if (out.data.size() != n) { printf("FAIL %s buffer %zu: %zu samples sent, want head(%zu)\n", k.name.c_str(), b, out.data.size(), n); failures++; }
    else
      for (size_t i = 0; i < n; i++)
        if (!same(out.data[i], y[off + i])) { printf("FAIL %s buffer %zu sample %zu\n", k.name.c_str(), b, i); failures++; break; }
    if (bitsOf(agc.gain()) != k.gain[b] || bitsOf(agc.level()) != k.sd[b]) {
      printf("FAIL %s buffer %zu: gain %08x level %08x, want %08x %08x\n", k.name.c_str(), b, bitsOf(agc.gain()), bitsOf(agc.level()), k.gain[b], k.sd[b]);
      failures++;
    }
    off += n;
    samples += n;
  }
  // config() again: the average starts over at the target, the gain stays
  const float g = agc.gain();
  src.configure(k.Fs, 4096);
  if (bitsOf(agc.gain()) != bitsOf(g) || agc.level() != (k.target ? float(k.target) : (sizeof(T) == 2 ? 16000.f : 0.5f))) {
    printf("FAIL %s: config() left gain %g level %g\n", k.name.c_str(), (double)agc.gain(), (double)agc.level());
    failures++;
  }
  return failures;
}

// The streams of one type are cut at two or three sample rates and a bank has one: the rows of equal rate share a bank, and every
// row runs through processDev on device rows of stride n + 8 whose 8 samples behind n must stay zero.
template <class T>
static int runBank(const std::vector<Case> &cases, const char *dtype, const std::string &dir) {
  const size_t n = 1024, stride = n + 8;
  std::vector<const Case *> rows;
  for (size_t i = 0; i < cases.size(); i++) if (cases[i].dtype == dtype) rows.push_back(&cases[i]);
  int failures = 0;
  size_t done = 0;
  for (size_t c0 = 0; c0 < rows.size(); c0++) {
    std::vector<const Case *> mine;
    bool first = true;
    for (size_t c = 0; c < rows.size(); c++)
      if (rows[c]->Fs == rows[c0]->Fs) { if (c < c0) first = false; mine.push_back(rows[c]); }
    if (!first) continue;
    const size_t C = mine.size(), bytes = C * stride * sizeof(T);
    std::vector<double> tau, target;
    std::vector<T> in(C * stride, T(0)), want(C * n), got(C * stride);
    for (size_t r = 0; r < C; r++) {
      tau.push_back(mine[r]->tau); target.push_back(mine[r]->target);
      std::vector<T> x = readBin<T>(dir + "/" + mine[r]->name + "_x.bin", mine[r]->count), y = readBin<T>(dir + "/" + mine[r]->name + "_y.bin", mine[r]->count);
      std::copy(x.begin(), x.begin() + n, in.begin() + r * stride);
      std::copy(y.begin(), y.begin() + n, want.begin() + r * n);
    }
    gpu::AGCBank<T> bank(mine[0]->Fs, tau, target, std::vector<bool>(C, true), n);
    void *din = 0, *dout = 0;
    if (sdrhip_malloc(bank.context(), bytes, &din) != SDRHIP_OK || sdrhip_malloc(bank.context(), bytes, &dout) != SDRHIP_OK) { printf("FAIL malloc\n"); return 1; }
    sdrhip_memcpy_h2d(bank.context(), din, in.data(), bytes);
    sdrhip_memset(bank.context(), dout, 0, bytes);
    if (!bank.processDev(static_cast<const T *>(din), n, stride, static_cast<T *>(dout), stride)) { printf("FAIL processDev\n"); failures++; }
    sdrhip_ctx_synchronize(bank.context());
    sdrhip_memcpy_d2h(bank.context(), got.data(), dout, bytes);
    sdrhip_free(bank.context(), din);
    sdrhip_free(bank.context(), dout);
    for (size_t r = 0; r < C; r++, done++) {
      for (size_t i = 0; i < n; i++)
        if (!same(got[r * stride + i], want[r * n + i])) { printf("FAIL processDev %s sample %zu\n", mine[r]->name.c_str(), i); failures++; break; }
      for (size_t i = n; i < stride; i++)
        if (!same(got[r * stride + i], T(0))) { printf("FAIL processDev %s wrote behind n\n", mine[r]->name.c_str()); failures++; break; }
    }
    std::vector<float> gain, level;
    bank.state(gain, level);
    for (size_t r = 0; r < C; r++)
      if (!(level[r] > 0) || gain.size() != C) { printf("FAIL state of %s\n", mine[r]->name.c_str()); failures++; }
  }
  printf("processDev %s: %zu rows\n", dtype, done);
  return failures;
}

// setTau between two buffers: tau() answers the new value, gain and level stay what they were, and the second buffer runs with the
// new decay from the state the first one left.
template <class T>
static int runTau(std::istringstream &s, const std::string &name, const std::string &dir) {
  double Fs, tau, target, tau2;
  size_t n1, n2;
  uint32_t g1, s1, g2, s2;
  std::string expected;
  s >> Fs >> tau >> target >> tau2 >> n1 >> n2 >> g1 >> s1 >> g2 >> s2 >> expected;
  if (!s) { printf("FAIL bad tau line\n"); return 1; }
  std::vector<T> x = readBin<T>(dir + "/" + name + "_x.bin", n1 + n2), y = readBin<T>(expected, n1 + n2);
  Feeder<T> src;
  gpu::AGC<T> agc(tau, target);
  Capture<T> out;
  src.connect(&agc, true); agc.connect(&out, true);
  src.configure(Fs, 8192);
  int failures = 0;
  src.feed(x.data(), n1);
  bool ok = out.data.size() == n1;
  for (size_t i = 0; ok && i < n1; i++) ok = same(out.data[i], y[i]);
  if (!ok || bitsOf(agc.gain()) != g1 || bitsOf(agc.level()) != s1) { printf("FAIL setTau %s: first buffer\n", name.c_str()); failures++; }
  agc.setTau(tau2);
  if (agc.tau() != double(float(tau2)) || bitsOf(agc.gain()) != g1 || bitsOf(agc.level()) != s1) { printf("FAIL setTau %s: the setter moved the state\n", name.c_str()); failures++; }
  src.feed(x.data() + n1, n2);
  ok = out.data.size() == n2;
  for (size_t i = 0; ok && i < n2; i++) ok = same(out.data[i], y[n1 + i]);
  if (!ok || bitsOf(agc.gain()) != g2 || bitsOf(agc.level()) != s2) {
    printf("FAIL setTau %s: second buffer, gain %08x level %08x, want %08x %08x\n", name.c_str(), bitsOf(agc.gain()), bitsOf(agc.level()), g2, s2);
    failures++;
  }
  printf("setTau %s: %zu + %zu samples\n", name.c_str(), n1, n2);
  return failures;
}

int main(int argc, char **argv) {
  if (argc < 4) { fprintf(stderr, "usage: test_agc <cases.txt> <golden dir> <tau.txt>\n"); return 2; }
  std::vector<Case> cases;
  std::ifstream f(argv[1]);
  std::string line;
  while (std::getline(f, line)) {
    if (line.empty()) continue;
    std::istringstream s(line);
    Case k;
    size_t nl, no;
    s >> k.name >> k.dtype >> k.Fs >> k.tau >> k.target >> k.count >> nl;
    k.lens.resize(nl);
    for (size_t i = 0; i < nl; i++) s >> k.lens[i];
    s >> no;
    k.ops.resize(no);
    for (size_t i = 0; i < no; i++) s >> k.ops[i].at >> k.ops[i].what >> k.ops[i].bits;
    k.gain.resize(nl); k.sd.resize(nl);
    for (size_t i = 0; i < nl; i++) s >> k.gain[i] >> k.sd[i];
    if (!s) { fprintf(stderr, "bad case line: %s\n", line.c_str()); return 2; }
    cases.push_back(k);
  }
  const std::string dir = argv[2];
  int failures = 0;
  size_t samples = 0;
  try {
    for (size_t i = 0; i < cases.size(); i++)
      failures += cases[i].dtype == "i16" ? runNode<int16_t>(cases[i], dir, samples) : runNode<float>(cases[i], dir, samples);
    printf("nodes: %zu streams, %zu samples\n", cases.size(), samples);
    failures += runBank<int16_t>(cases, "i16", dir);
    failures += runBank<float>(cases, "f32", dir);
    std::ifstream tf(argv[3]);
    size_t taus = 0;
    while (std::getline(tf, line)) {
      if (line.empty()) continue;
      std::istringstream ts(line);
      std::string name, dtype;
      ts >> name >> dtype;
      failures += dtype == "i16" ? runTau<int16_t>(ts, name, dir) : runTau<float>(ts, name, dir);
      taus++;
    }
    if (taus != 2) { printf("FAIL %zu setTau cases, want 2\n", taus); failures++; }
  } catch (const std::exception &e) {
    printf("FAIL exception: %s\n", e.what());
    failures++;
  }
  printf("%s (%d failures)\n", failures ? "FAILED" : "OK", failures);
  return failures ? 1 : 0;
}
