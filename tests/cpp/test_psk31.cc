// test_psk31.cc — sdr::gpu::BPSK31<int16_t>, gpu::BPSK31<float>, gpu::BPSK31Bank and the host-only sdr::Varicode
// (include/sdr/gpu/psk31.hh).
//   test_psk31 varicode <bits.bin> <nbits> <text.bin> <nchars>
//       host only: the bit stream through Source -> Varicode -> Sink in ragged buffers that end inside codes
//   test_psk31 nodes <cases.txt> <golden dir> <table.bin>
//       on the GPU: every g21_psk31_* stream through Source -> gpu::BPSK31 -> Sink in its recorded buffers, with the reference's
//       table, against the reference's bits and per-buffer counts; the config rules; then the first buffers of the streams of a
//       type and sample rate as the rows of one BPSK31Bank, through host pointers and as strided device rows.
// cases.txt, one stream per line: name dtype Fs dF count nbits  nlens lens...  counts...
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "sdr/gpu/psk31.hh"

using namespace sdr;

struct Case {
  std::string name, dtype;
  double Fs, dF;
  size_t count, nbits;
  std::vector<size_t> lens, counts;
};

template <class T>
static std::vector<T> readBin(const std::string &path, size_t count) {
  std::vector<T> v(count);
  std::ifstream f(path.c_str(), std::ios::binary);
  f.read(reinterpret_cast<char *>(v.data()), count * sizeof(T));
  if ((size_t)f.gcount() != count * sizeof(T)) { fprintf(stderr, "%s: short file\n", path.c_str()); exit(2); }
  return v;
}

class Capture : public Sink<uint8_t> {
public:
  std::vector<uint8_t> data;
  Config cfg;
  virtual void config(const Config &c) { cfg = c; }
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

static int runVaricode(const std::string &bitsFile, size_t nbits, const std::string &textFile, size_t nchars) {
  std::vector<uint8_t> bits = readBin<uint8_t>(bitsFile, nbits), text = readBin<uint8_t>(textFile, nchars);
  Feeder<uint8_t> src;
  Varicode node;
  Capture out;
  src.connect(&node, true); node.connect(&out, true);
  src.configure(31.25, 64);
  const size_t pattern[] = {64, 1, 7, 13, 2, 17, 5, 11, 3, 40};
  size_t off = 0, k = 0;
  while (off < nbits) {
    const size_t len = std::min(pattern[k++ % 10], nbits - off);
    src.feed(bits.data() + off, len);
    off += len;
  }
  int failures = 0;
  if (out.data != text) { printf("FAIL varicode: %zu characters, want %zu\n", out.data.size(), text.size()); failures++; }
  if (out.cfg.type() != Config::typeId<uint8_t>()) { printf("FAIL varicode: output type\n"); failures++; }
  // a wrong input type is a ConfigError
  bool threw = false;
  try {
    Feeder<int16_t> bad;
    Varicode v;
    bad.connect(&v, true);
    bad.configure(31.25, 64);
  } catch (ConfigError &) { threw = true; }
  if (!threw) { printf("FAIL varicode: an int16 input was accepted\n"); failures++; }
  printf("varicode: %zu bits, %zu characters\n", nbits, out.data.size());
  return failures;
}

template <class T>
static int runNode(const Case &k, const std::string &dir, const std::vector<float> &table) {
  typedef std::complex<T> CT;
  std::vector<CT> x = readBin<CT>(dir + "/" + k.name + "_x.bin", k.count);
  std::vector<uint8_t> want = readBin<uint8_t>(dir + "/" + k.name + "_bits.bin", k.nbits);
  Feeder<CT> src;
  gpu::BPSK31<T> node(k.dF, table.data());
  Capture out;
  src.connect(&node, true); node.connect(&out, true);
  src.configure(k.Fs, (size_t)k.Fs);
  int failures = 0;
  if (out.cfg.type() != Config::typeId<uint8_t>() || out.cfg.sampleRate() != 31.25) { printf("FAIL %s: output config\n", k.name.c_str()); failures++; }
  size_t off = 0;
  for (size_t b = 0; b < k.lens.size(); b++) {
    const size_t before = out.data.size();
    src.feed(x.data() + off, k.lens[b]);
    off += k.lens[b];
    if (out.data.size() - before != k.counts[b]) {
      printf("FAIL %s buffer %zu: %zu bits, want %zu\n", k.name.c_str(), b, out.data.size() - before, k.counts[b]);
      failures++;
    }
  }
  if (out.data != want) { printf("FAIL %s: the bits differ from the reference's\n", k.name.c_str()); failures++; }
  float P, F, mu, omega;
  node.state(P, F, mu, omega);
  if (!(mu > 0) || !(omega > 0)) { printf("FAIL %s: state mu %g omega %g\n", k.name.c_str(), (double)mu, (double)omega); failures++; }
  return failures;
}

template <class T>
static int configRules() {
  int failures = 0;
  bool threw = false;
  try {   // below 2000 Hz
    Feeder< std::complex<T> > src;
    gpu::BPSK31<T> node;
    src.connect(&node, true);
    src.configure(1999.0, 512);
  } catch (ConfigError &) { threw = true; }
  if (!threw) { printf("FAIL config: 1999 Hz was accepted\n"); failures++; }
  threw = false;
  try {   // the other scalar type
    Feeder< std::complex<double> > src;
    gpu::BPSK31<T> node;
    src.connect(&node, true);
    src.configure(8000.0, 512);
  } catch (ConfigError &) { threw = true; }
  if (!threw) { printf("FAIL config: a complex<double> input was accepted\n"); failures++; }
  return failures;
}

// the first buffer of every stream of one type and sample rate: rows of one bank, host pointers and strided device rows
template <class T>
static int runBank(const std::vector<Case> &cases, const char *dtype, double Fs, const std::string &dir, const std::vector<float> &table) {
  typedef std::complex<T> CT;
  std::vector<const Case *> rows;
  for (size_t i = 0; i < cases.size(); i++) if (cases[i].dtype == dtype && cases[i].Fs == Fs) rows.push_back(&cases[i]);
  if (rows.empty()) return 0;
  const size_t C = rows.size(), n = rows[0]->lens[0], stride = n + 8;
  std::vector<CT> x(C * stride);
  std::vector<float> dF(C);
  for (size_t c = 0; c < C; c++) {
    std::vector<CT> r = readBin<CT>(dir + "/" + rows[c]->name + "_x.bin", rows[c]->count);
    std::copy(r.begin(), r.begin() + n, x.begin() + c * stride);
    dF[c] = (float)rows[c]->dF;
  }
  int failures = 0;
  gpu::BPSK31Bank<T> host(Fs, dF, n, table.data()), dev(Fs, dF, n, table.data());
  const size_t cap = host.capacity(n), ostride = cap + 5;
  std::vector<uint8_t> bits(C * ostride, 9), dbits(C * ostride, 7);
  std::vector<uint32_t> counts(C, 99), dcounts(C, 98);
  if (!host.process(x.data(), n, stride, bits.data(), ostride, counts.data())) { printf("FAIL bank %s: process\n", dtype); return 1; }
  void *din = 0, *dout = 0, *dcnt = 0;
  sdrhip_ctx *ctx = dev.context();
  if (sdrhip_malloc(ctx, x.size() * sizeof(CT), &din) || sdrhip_malloc(ctx, dbits.size(), &dout) || sdrhip_malloc(ctx, C * 4, &dcnt)) return 1;
  sdrhip_memcpy_h2d(ctx, din, x.data(), x.size() * sizeof(CT));
  sdrhip_memcpy_h2d(ctx, dout, dbits.data(), dbits.size());
  if (!dev.processDev(din, n, stride, static_cast<uint8_t *>(dout), ostride, static_cast<uint32_t *>(dcnt))) { printf("FAIL bank %s: processDev\n", dtype); failures++; }
  sdrhip_ctx_synchronize(ctx);
  sdrhip_memcpy_d2h(ctx, dbits.data(), dout, dbits.size());
  sdrhip_memcpy_d2h(ctx, dcounts.data(), dcnt, C * 4);
  for (size_t c = 0; c < C; c++) {
    std::vector<uint8_t> want = readBin<uint8_t>(dir + "/" + rows[c]->name + "_bits.bin", rows[c]->nbits);
    if (counts[c] != rows[c]->counts[0] || dcounts[c] != counts[c]) {
      printf("FAIL bank %s row %zu: counts %u / %u, want %zu\n", dtype, c, counts[c], dcounts[c], rows[c]->counts[0]);
      failures++;
      continue;
    }
    if (memcmp(&bits[c * ostride], want.data(), counts[c]) || memcmp(&dbits[c * ostride], want.data(), counts[c])) {
      printf("FAIL bank %s row %zu: bits\n", dtype, c);
      failures++;
    }
    for (size_t i = cap; i < ostride; i++)   // behind the capacity a row is the caller's
      if (bits[c * ostride + i] != 9 || dbits[c * ostride + i] != 7) { printf("FAIL bank %s row %zu: byte %zu behind the capacity was written\n", dtype, c, i); failures++; break; }
  }
  sdrhip_free(ctx, din); sdrhip_free(ctx, dout); sdrhip_free(ctx, dcnt);
  printf("bank %s at %g Hz: %zu rows\n", dtype, Fs, C);
  return failures;
}

int main(int argc, char **argv) {
  if (argc >= 6 && std::string(argv[1]) == "varicode") {
    const int failures = runVaricode(argv[2], (size_t)atol(argv[3]), argv[4], (size_t)atol(argv[5]));
    printf("%s (%d failures)\n", failures ? "FAILED" : "OK", failures);
    return failures ? 1 : 0;
  }
  if (argc < 5 || std::string(argv[1]) != "nodes") { fprintf(stderr, "usage: test_psk31 varicode ... | nodes <cases.txt> <golden dir> <table.bin>\n"); return 2; }
  std::vector<Case> cases;
  std::ifstream f(argv[2]);
  std::string line;
  while (std::getline(f, line)) {
    std::istringstream s(line);
    Case k;
    size_t nl = 0;
    s >> k.name >> k.dtype >> k.Fs >> k.dF >> k.count >> k.nbits >> nl;
    if (!s) continue;
    k.lens.resize(nl); k.counts.resize(nl);
    for (size_t i = 0; i < nl; i++) s >> k.lens[i];
    for (size_t i = 0; i < nl; i++) s >> k.counts[i];
    cases.push_back(k);
  }
  const std::string dir = argv[3];
  const std::vector<float> table = readBin<float>(argv[4], 129 * 8);
  int failures = 0;
  try {
    for (size_t i = 0; i < cases.size(); i++)
      failures += cases[i].dtype == "cs16" ? runNode<int16_t>(cases[i], dir, table) : runNode<float>(cases[i], dir, table);
    printf("nodes: %zu streams\n", cases.size());
    failures += configRules<int16_t>() + configRules<float>();
    failures += runBank<int16_t>(cases, "cs16", 8000.0, dir, table) + runBank<float>(cases, "cf32", 8000.0, dir, table);
    failures += runBank<float>(cases, "cf32", 2000.0, dir, table);
  } catch (SDRError &e) {
    printf("FAIL exception: %s\n", e.what());
    failures++;
  }
  printf("%s (%d failures)\n", failures ? "FAILED" : "OK", failures);
  return failures ? 1 : 0;
}
