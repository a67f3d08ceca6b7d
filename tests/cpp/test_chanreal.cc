// test_chanreal.cc — sdr::gpu::RealChannelizer<Scalar>, RealAudioChannelizer<Scalar>, RealChannelPower<Scalar>
// (include/sdr/gpu/chanreal.hh).
//   test_chanreal rules
//       host only: the three constructors' rules and the setters' throw ConfigError, and config() refuses another input type
//       before it looks for a device
//   test_chanreal audio <case.txt> <taps.bin> <x.bin> <want.bin> <want_one.bin>
//       on the GPU: the stream through Source -> gpu::RealAudioChannelizer<int16_t> -> one Sink per row, buffer by buffer, bit
//       for bit the int16 rows the Python node gave for the same buffers (want.bin: rows x (n / D) int16), then as one device
//       row through processDev, bit for bit the Python node's one call (want_one.bin); row i has mode (FM, AM, USB)[i % 3] and
//       gain 0.75 + 0.5 i
//   test_chanreal power <case.txt> <taps.bin> <x.bin> <want.bin>
//       on the GPU: the stream through Source -> gpu::RealChannelPower<int16_t>, buffer by buffer, against the Python node's
//       figures for the same buffers, bit for bit (want.bin, doubles: the open threshold (close is half of it), then K sums
//       of the last buffer, K levels, K flags, and K sums of the whole stream in one call, which processDev is held to)
//   test_chanreal graph <case.txt> <taps.bin> <x.bin> <want.bin>
//       on the GPU: a real int16 stream through Source -> gpu::RealChannelizer<int16_t> -> one Sink per selected row, in the
//       buffers the case lists, against the values the Python side wrote from the numpy restatement: max |y - want| / max |want|
//       <= 1e-5 over all rows; the per-buffer output counts and the output Config; then the same stream as device rows through
//       processDev on a second node, bit for bit the graph's values.
// case.txt: M D n_taps n rows  channel...  nbuf len...      taps.bin: n_taps doubles; x.bin: n x int16;
// want.bin: rows x (n / D) x (double re, im)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "sdr/gpu/chanreal.hh"
#include "harness.hh"

typedef int16_t cs;   // the real row's element
typedef std::complex<float> cf;

static int runRules() {
  int failures = 0, n = 0;
  const std::vector<double> t24(24, 0.04);
  std::vector<double> bad = t24;
  bad[7] = HUGE_VAL;
  std::vector<double> huge = t24;
  huge[7] = 1e39;   // finite as a double, not as a float
#define REFUSED(...) do { n++; if (!refused([&] { __VA_ARGS__; })) { printf("FAIL rules: accepted: %s\n", #__VA_ARGS__); failures++; } } while (0)
  REFUSED(gpu::RealChannelizer<int16_t> c(2, 1, t24));
  REFUSED(gpu::RealChannelizer<int16_t> c(4098, 8, t24));
  REFUSED(gpu::RealChannelizer<int16_t> c(9, 8, t24));
  REFUSED(gpu::RealChannelizer<int16_t> c(34, 8, t24));
  REFUSED(gpu::RealChannelizer<float> c(4 * 19, 8, t24));
  REFUSED(gpu::RealChannelizer<int16_t> c(8, 0, t24));
  REFUSED(gpu::RealChannelizer<int16_t> c(8, 9, t24));
  REFUSED(gpu::RealChannelizer<int16_t> c(8, 4, std::vector<double>()));
  REFUSED(gpu::RealChannelizer<int16_t> c(4, 1, std::vector<double>(257, 0.1)));
  REFUSED(gpu::RealChannelizer<float> c(8, 4, bad));
  REFUSED(gpu::RealChannelizer<int16_t> c(8, 4, huge));
  REFUSED(gpu::RealChannelizer<int16_t> c(8, 4, t24, std::vector<int>(1, 5)));
  REFUSED(gpu::RealChannelizer<int16_t> c(8, 4, t24, std::vector<int>(1, -1)));
  REFUSED(gpu::RealChannelizer<int16_t> c(8, 4, t24, std::vector<int>(2, 3)));
#undef REFUSED
  // what the rules admit constructs without a device
  if (refused([&] { gpu::RealChannelizer<int16_t> a(8, 4, t24), b(4096, 4096, std::vector<double>(5, 0.2)), c(1000, 1, t24, std::vector<int>(1, 500)), d(26, 13, t24), e(4, 4, t24); })) {
    printf("FAIL rules: a valid node was refused\n");
    failures++;
  }
  gpu::RealChannelizer<float> all(12, 6, t24);
  if (all.rows() != 7 || all.channel(6) != 6 || all.source(6) == 0) { printf("FAIL rules: the default selection\n"); failures++; }
  printf("rules: %d constructions refused\n", n);
  // the audio node: the same rules, and a mode and a gain per row
  const std::vector<int> none;
  const std::vector<float> nog;
  n = 0;
#define REFUSED(...) do { n++; if (!refused([&] { __VA_ARGS__; })) { printf("FAIL rules: accepted: %s\n", #__VA_ARGS__); failures++; } } while (0)
  REFUSED(gpu::RealAudioChannelizer<int16_t> c(2, 1, t24));
  REFUSED(gpu::RealAudioChannelizer<int16_t> c(9, 8, t24));
  REFUSED(gpu::RealAudioChannelizer<float> c(34, 8, t24));
  REFUSED(gpu::RealAudioChannelizer<int16_t> c(8, 9, t24));
  REFUSED(gpu::RealAudioChannelizer<int16_t> c(8, 4, bad));
  REFUSED(gpu::RealAudioChannelizer<int16_t> c(8, 4, t24, std::vector<int>(1, 5)));
  REFUSED(gpu::RealAudioChannelizer<int16_t> c(8, 4, t24, none, std::vector<int>(8, int(SDRHIP_EPI_FM))));       // M modes, K = 5 rows
  REFUSED(gpu::RealAudioChannelizer<int16_t> c(8, 4, t24, none, std::vector<int>(5, int(SDRHIP_EPI_NONE))));
  REFUSED(gpu::RealAudioChannelizer<int16_t> c(8, 4, t24, none, none, std::vector<float>(5, float(HUGE_VAL))));
  REFUSED(gpu::RealAudioChannelizer<int16_t> c(8, 4, t24, none, none, std::vector<float>(4, 1.f)));
  printf("rules: audio: %d constructions refused\n", n);
  gpu::RealAudioChannelizer<float> audio(12, 6, t24, none, std::vector<int>(7, int(SDRHIP_EPI_USB)), std::vector<float>(7, 2.f));
  if (audio.rows() != 7 || audio.channel(6) != 6 || audio.mode(6) != SDRHIP_EPI_USB || audio.gain(0) != 2.f || audio.source(6) == 0) {
    printf("FAIL rules: the audio node's default selection\n");
    failures++;
  }
  // the monitor: the same rules and alpha; K thresholds
  n = 0;
  REFUSED(gpu::RealChannelPower<int16_t> c(2, 1, t24));
  REFUSED(gpu::RealChannelPower<int16_t> c(9, 8, t24));
  REFUSED(gpu::RealChannelPower<float> c(34, 8, t24));
  REFUSED(gpu::RealChannelPower<int16_t> c(8, 0, t24));
  REFUSED(gpu::RealChannelPower<int16_t> c(8, 4, huge));
  REFUSED(gpu::RealChannelPower<int16_t> c(8, 4, t24, 0.0));
  REFUSED(gpu::RealChannelPower<int16_t> c(8, 4, t24, 1.5));
  gpu::RealChannelPower<int16_t> mon(8, 4, t24, 0.5);
  REFUSED(mon.setThresholds(std::vector<double>(8, 2.0), std::vector<double>(8, 1.0)));                         // M values, K = 5 channels
  REFUSED(mon.setThresholds(1.0, 2.0));
  REFUSED(mon.setAlpha(0.0));
  REFUSED(mon.setTaps(std::vector<double>(23, 0.1)));
#undef REFUSED
  printf("rules: power: %d refused\n", n);
  if (refused([&] { mon.setThresholds(std::vector<double>(5, 2.0), std::vector<double>(5, 1.0)); mon.setThresholds(3.0, 1.0); }) ||
      mon.channels() != 5 || mon.sums().size() != 5 || mon.levels().size() != 5 || mon.open().size() != 5 || !mon.occupied().empty()) {
    printf("FAIL rules: the monitor's K = 5 channels\n");
    failures++;
  }
  // config(): another input type is refused before a device is looked for
  int typed = 0;
  {
    Feeder< std::complex<int16_t> > a, b, c;
    gpu::RealChannelizer<int16_t> n1(8, 4, t24);
    gpu::RealAudioChannelizer<int16_t> n2(8, 4, t24);
    gpu::RealChannelPower<int16_t> n3(8, 4, t24);
    a.connect(&n1, true); b.connect(&n2, true); c.connect(&n3, true);
    typed += refused([&] { a.configure(48000.0, 512); });
    typed += refused([&] { b.configure(48000.0, 512); });
    typed += refused([&] { c.configure(48000.0, 512); });
    Feeder<float> d;
    gpu::RealChannelizer<int16_t> n4(8, 4, t24);
    d.connect(&n4, true);
    typed += refused([&] { d.configure(48000.0, 512); });
  }
  if (typed != 4) { printf("FAIL rules: config() accepted another input type (%d of 4 refused)\n", typed); failures++; }
  printf("rules: config: %d input types refused\n", typed);
  return failures;
}

static int runGraph(const char *casePath, const char *tapsPath, const char *xPath, const char *wantPath) {
  std::ifstream f(casePath);
  size_t M = 0, D = 0, nTaps = 0, n = 0, rows = 0, nbuf = 0;
  f >> M >> D >> nTaps >> n >> rows;
  std::vector<int> sel(rows);
  for (size_t i = 0; i < rows; i++) f >> sel[i];
  f >> nbuf;
  std::vector<size_t> lens(nbuf);
  for (size_t i = 0; i < nbuf; i++) f >> lens[i];
  if (!f) { fprintf(stderr, "%s: bad case file\n", casePath); return 1; }
  const std::vector<double> taps = readBin<double>(tapsPath, nTaps);
  std::vector<cs> x = readBin<cs>(xPath, n);
  const size_t no = n / D;
  const std::vector<double> want = readBin<double>(wantPath, rows * no * 2);
  size_t bs = 0;
  for (size_t i = 0; i < nbuf; i++) bs = std::max(bs, lens[i]);

  int failures = 0;
  Feeder<cs> src;
  gpu::RealChannelizer<int16_t> node(M, D, taps, sel);
  std::vector< Capture<cf> > outs(rows);
  src.connect(&node, true);
  for (size_t i = 0; i < rows; i++) node.source(i)->connect(&outs[i], true);
  const double Fs = 48000.0;
  src.configure(Fs, bs);
  const size_t stride = (bs + D - 1) / D;
  for (size_t i = 0; i < rows; i++)
    if (outs[i].cfg.type() != Config::typeId<cf>() || outs[i].cfg.sampleRate() != Fs / double(D) || outs[i].cfg.bufferSize() != stride) {
      printf("FAIL graph row %zu: output config (rate %g, buffer %zu)\n", i, outs[i].cfg.sampleRate(), outs[i].cfg.bufferSize());
      failures++;
    }
  size_t off = 0;
  for (size_t b = 0; b < nbuf; b++) {
    const size_t before = outs[0].data.size(), count = (off + lens[b]) / D - off / D;
    src.feed(x.data() + off, lens[b]);
    off += lens[b];
    for (size_t i = 0; i < rows; i++)
      if (outs[i].data.size() - before != count) { printf("FAIL graph buffer %zu row %zu: %zu outputs, want %zu\n", b, i, outs[i].data.size() - before, count); failures++; }
  }
  if (node.consumed() != n) { printf("FAIL graph: consumed %llu\n", (unsigned long long)node.consumed()); failures++; }
  double worst = 0, scale = 0;
  for (size_t i = 0; i < rows; i++) {
    if (outs[i].data.size() != no) { printf("FAIL graph row %zu: %zu outputs in all, want %zu\n", i, outs[i].data.size(), no); return failures + 1; }
    for (size_t j = 0; j < no; j++) {
      const double wr = want[(i * no + j) * 2], wi = want[(i * no + j) * 2 + 1];
      worst = std::max(worst, std::hypot(double(outs[i].data[j].real()) - wr, double(outs[i].data[j].imag()) - wi));
      scale = std::max(scale, std::hypot(wr, wi));
    }
  }
  printf("graph: %zu rows x %zu outputs, max |y - want| / max |want| = %.3g\n", rows, no, worst / scale);
  if (!(worst <= 1e-5 * scale)) { printf("FAIL graph: above 1e-5\n"); failures++; }

  // the same stream as device rows, one call, on a node of its own
  Feeder<cs> src2;
  gpu::RealChannelizer<int16_t> dev(M, D, taps, sel);
  src2.connect(&dev, true);
  src2.configure(Fs, n);
  sdrhip_ctx *ctx = dev.context();
  const size_t dstride = no + 5;
  std::vector<cf> host(rows * dstride, cf(7.f, 7.f));
  void *din = 0, *dout = 0;
  if (sdrhip_malloc(ctx, n * sizeof(cs), &din) || sdrhip_malloc(ctx, host.size() * sizeof(cf), &dout)) return failures + 1;
  sdrhip_memcpy_h2d(ctx, din, x.data(), n * sizeof(cs));
  sdrhip_memcpy_h2d(ctx, dout, host.data(), host.size() * sizeof(cf));
  size_t got = 0;
  if (!dev.processDev(din, n, dout, dstride, &got) || got != no) { printf("FAIL processDev: %zu outputs\n", got); failures++; }
  sdrhip_ctx_synchronize(ctx);
  sdrhip_memcpy_d2h(ctx, host.data(), dout, host.size() * sizeof(cf));
  for (size_t i = 0; i < rows; i++) {
    if (memcmp(&host[i * dstride], outs[i].data.data(), no * sizeof(cf))) { printf("FAIL processDev row %zu differs from the graph's\n", i); failures++; }
    for (size_t j = no; j < dstride; j++)
      if (host[i * dstride + j] != cf(7.f, 7.f)) { printf("FAIL processDev row %zu: element %zu behind the count was written\n", i, j); failures++; break; }
  }
  sdrhip_free(ctx, din); sdrhip_free(ctx, dout);
  printf("processDev: %zu rows\n", rows);

  return failures;
}

struct Case {
  size_t M, D, nTaps, n, rows, no;
  std::vector<int> sel;
  std::vector<size_t> lens;
  size_t bs;
};

static bool readCase(const char *path, Case &c) {
  std::ifstream f(path);
  size_t nbuf = 0;
  f >> c.M >> c.D >> c.nTaps >> c.n >> c.rows;
  c.sel.resize(c.rows);
  for (size_t i = 0; i < c.rows; i++) f >> c.sel[i];
  f >> nbuf;
  c.lens.resize(nbuf);
  c.bs = 0;
  for (size_t i = 0; i < nbuf; i++) { f >> c.lens[i]; c.bs = std::max(c.bs, c.lens[i]); }
  c.no = c.D ? c.n / c.D : 0;
  if (!f) fprintf(stderr, "%s: bad case file\n", path);
  return bool(f);
}

static int runAudio(const char *casePath, const char *tapsPath, const char *xPath, const char *wantPath, const char *onePath) {
  Case c;
  if (!readCase(casePath, c)) return 1;
  const std::vector<double> taps = readBin<double>(tapsPath, c.nTaps);
  std::vector<cs> x = readBin<cs>(xPath, c.n);
  const std::vector<int16_t> want = readBin<int16_t>(wantPath, c.rows * c.no), one = readBin<int16_t>(onePath, c.rows * c.no);
  const int codes[3] = {SDRHIP_EPI_FM, SDRHIP_EPI_AM, SDRHIP_EPI_USB};
  std::vector<int> modes(c.rows);
  std::vector<float> gains(c.rows);
  for (size_t i = 0; i < c.rows; i++) { modes[i] = codes[i % 3]; gains[i] = 0.75f + 0.5f * float(i); }
  int failures = 0;
  Feeder<cs> src;
  gpu::RealAudioChannelizer<int16_t> node(c.M, c.D, taps, c.sel, modes, gains);
  std::vector< Capture<int16_t> > outs(c.rows);
  src.connect(&node, true);
  for (size_t i = 0; i < c.rows; i++) node.source(i)->connect(&outs[i], true);
  const double Fs = 48000.0;
  src.configure(Fs, c.bs);
  const size_t stride = (c.bs + c.D - 1) / c.D;
  for (size_t i = 0; i < c.rows; i++)
    if (outs[i].cfg.type() != Config::typeId<int16_t>() || outs[i].cfg.sampleRate() != Fs / double(c.D) || outs[i].cfg.bufferSize() != stride) {
      printf("FAIL audio row %zu: output config\n", i);
      failures++;
    }
  size_t off = 0;
  for (size_t b = 0; b < c.lens.size(); b++) { src.feed(x.data() + off, c.lens[b]); off += c.lens[b]; }
  if (node.consumed() != c.n) { printf("FAIL audio: consumed %llu\n", (unsigned long long)node.consumed()); failures++; }
  for (size_t i = 0; i < c.rows; i++) {
    if (outs[i].data.size() != c.no) { printf("FAIL audio row %zu: %zu outputs, want %zu\n", i, outs[i].data.size(), c.no); return failures + 1; }
    if (memcmp(outs[i].data.data(), &want[i * c.no], c.no * sizeof(int16_t))) { printf("FAIL audio row %zu differs\n", i); failures++; }
  }
  printf("audio: %zu rows x %zu outputs\n", c.rows, c.no);
  // one device row through processDev on a node of its own
  Feeder<cs> src2;
  gpu::RealAudioChannelizer<int16_t> dev(c.M, c.D, taps, c.sel, modes, gains);
  src2.connect(&dev, true);
  src2.configure(Fs, c.n);
  sdrhip_ctx *ctx = dev.context();
  const size_t dstride = c.no + 5;
  std::vector<int16_t> host(c.rows * dstride, int16_t(7));
  void *din = 0, *dout = 0;
  if (sdrhip_malloc(ctx, c.n * sizeof(cs), &din) || sdrhip_malloc(ctx, host.size() * sizeof(int16_t), &dout)) return failures + 1;
  sdrhip_memcpy_h2d(ctx, din, x.data(), c.n * sizeof(cs));
  sdrhip_memcpy_h2d(ctx, dout, host.data(), host.size() * sizeof(int16_t));
  size_t got = 0;
  if (!dev.processDev(din, c.n, dout, dstride, &got) || got != c.no) { printf("FAIL audio processDev: %zu outputs\n", got); failures++; }
  sdrhip_ctx_synchronize(ctx);
  sdrhip_memcpy_d2h(ctx, host.data(), dout, host.size() * sizeof(int16_t));
  for (size_t i = 0; i < c.rows; i++) {
    if (memcmp(&host[i * dstride], &one[i * c.no], c.no * sizeof(int16_t))) { printf("FAIL audio processDev row %zu differs\n", i); failures++; }
    for (size_t j = c.no; j < dstride; j++)
      if (host[i * dstride + j] != 7) { printf("FAIL audio processDev row %zu: element %zu behind the count was written\n", i, j); failures++; break; }
  }
  sdrhip_free(ctx, din); sdrhip_free(ctx, dout);
  printf("audio processDev: %zu rows\n", c.rows);
  return failures;
}

static int runPower(const char *casePath, const char *tapsPath, const char *xPath, const char *wantPath) {
  Case c;
  if (!readCase(casePath, c)) return 1;
  const size_t K = c.M / 2 + 1;
  const std::vector<double> taps = readBin<double>(tapsPath, c.nTaps);
  std::vector<cs> x = readBin<cs>(xPath, c.n);
  const std::vector<double> want = readBin<double>(wantPath, 1 + 4 * K);
  const double thr = want[0], *sums = &want[1], *levels = &want[1 + K], *flags = &want[1 + 2 * K], *one = &want[1 + 3 * K];
  int failures = 0;
  Feeder<cs> src;
  gpu::RealChannelPower<int16_t> node(c.M, c.D, taps, 0.375);
  node.setThresholds(thr, 0.5 * thr);
  src.connect(&node, true);
  src.configure(48000.0, c.bs);
  size_t off = 0, calls = 0;
  for (size_t b = 0; b < c.lens.size(); b++) {
    src.feed(x.data() + off, c.lens[b]);
    calls += ((off + c.lens[b]) / c.D - off / c.D) > 0;
    off += c.lens[b];
  }
  if (node.consumed() != c.n || node.calls() != calls) { printf("FAIL power: consumed %llu, calls %llu\n", (unsigned long long)node.consumed(), (unsigned long long)node.calls()); failures++; }
  const std::vector<double> lv = node.levels();
  const std::vector<bool> op = node.open();
  std::vector<int> occ;
  for (size_t k = 0; k < K; k++) if (flags[k] != 0.0) occ.push_back(int(k));
  if (node.channels() != K || node.sums().size() != K || lv.size() != K || op.size() != K) { printf("FAIL power: sizes\n"); return failures + 1; }
  if (memcmp(node.sums().data(), sums, K * sizeof(double))) { printf("FAIL power: the last buffer's sums differ\n"); failures++; }
  if (memcmp(lv.data(), levels, K * sizeof(double))) { printf("FAIL power: levels differ\n"); failures++; }
  for (size_t k = 0; k < K; k++) if (op[k] != (flags[k] != 0.0)) { printf("FAIL power: flag %zu\n", k); failures++; break; }
  if (node.occupied() != occ || occ.empty() || occ.size() == K) { printf("FAIL power: occupied (%zu open)\n", occ.size()); failures++; }
  printf("power: %zu channels, %zu open\n", K, occ.size());
  // one device row through processDev on a node of its own
  Feeder<cs> src2;
  gpu::RealChannelPower<int16_t> dev(c.M, c.D, taps, 0.375);
  src2.connect(&dev, true);
  src2.configure(48000.0, c.n);
  sdrhip_ctx *ctx = dev.context();
  std::vector<double> host(K + 3, 7.0);
  void *din = 0, *dsum = 0;
  if (sdrhip_malloc(ctx, c.n * sizeof(cs), &din) || sdrhip_malloc(ctx, host.size() * sizeof(double), &dsum)) return failures + 1;
  sdrhip_memcpy_h2d(ctx, din, x.data(), c.n * sizeof(cs));
  sdrhip_memcpy_h2d(ctx, dsum, host.data(), host.size() * sizeof(double));
  size_t got = 0;
  if (!dev.processDev(din, c.n, static_cast<double *>(dsum), &got) || got != c.no) { printf("FAIL power processDev: %zu outputs\n", got); failures++; }
  sdrhip_ctx_synchronize(ctx);
  sdrhip_memcpy_d2h(ctx, host.data(), dsum, host.size() * sizeof(double));
  if (memcmp(host.data(), one, K * sizeof(double))) { printf("FAIL power processDev: sums differ\n"); failures++; }
  for (size_t j = K; j < host.size(); j++) if (host[j] != 7.0) { printf("FAIL power processDev: element %zu behind the K sums was written\n", j); failures++; break; }
  sdrhip_free(ctx, din); sdrhip_free(ctx, dsum);
  printf("power processDev: %zu sums\n", K);
  return failures;
}

int main(int argc, char **argv) {
  return runMain("usage: test_chanreal rules | graph|power <case.txt> <taps.bin> <x.bin> <want.bin> | audio ... <want_one.bin>\n", [&]() -> int {
    if (argc >= 2 && std::string(argv[1]) == "rules") return runRules();
    if (argc >= 6 && std::string(argv[1]) == "graph") return runGraph(argv[2], argv[3], argv[4], argv[5]);
    if (argc >= 7 && std::string(argv[1]) == "audio") return runAudio(argv[2], argv[3], argv[4], argv[5], argv[6]);
    if (argc >= 6 && std::string(argv[1]) == "power") return runPower(argv[2], argv[3], argv[4], argv[5]);
    return -1;
  });
}
