// test_chanpower.cc — sdr::gpu::ChannelPower<Scalar> (include/sdr/gpu/chanpower.hh).
//   test_chanpower rules
//       host only: the constructor's rules and the setters' throw ConfigError
//   test_chanpower graph <case.txt> <taps.bin> <x.bin> <want.bin>
//       on the GPU: a cs16 stream through Source -> gpu::ChannelPower<int16_t> in two buffers, against the values the Python side
//       wrote from the numpy restatement: the sums of each buffer and the levels behind it to 1e-5 of the largest, occupied()
//       exactly; reset() and the same two buffers again, bit for bit; processDev with no sums on a second node, the same state.
// case.txt: M D n_taps alpha open_thr close_thr  n0 n1  count0 occupied0...  count1 occupied1...
// taps.bin: n_taps doubles; x.bin: (n0 + n1) x (int16 re, im); want.bin: 2 x (M sums, M levels) doubles
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "sdr/gpu/chanpower.hh"
#include "harness.hh"

typedef std::complex<int16_t> cs;
typedef std::complex<float> cf;

static int runRules() {
  int failures = 0, n = 0;
  const std::vector<double> t24(24, 0.04);
  std::vector<double> bad = t24;
  bad[7] = HUGE_VAL;
  std::vector<double> huge = t24;
  huge[7] = 1e39;   // finite as a double, not as a float
#define REFUSED(...) do { n++; if (!refused([&] { __VA_ARGS__; })) { printf("FAIL rules: accepted: %s\n", #__VA_ARGS__); failures++; } } while (0)
  REFUSED(gpu::ChannelPower<int16_t> c(1, 1, t24));
  REFUSED(gpu::ChannelPower<int16_t> c(4097, 8, t24));
  REFUSED(gpu::ChannelPower<int16_t> c(17, 8, t24));
  REFUSED(gpu::ChannelPower<float> c(38, 8, t24));
  REFUSED(gpu::ChannelPower<int16_t> c(8, 0, t24));
  REFUSED(gpu::ChannelPower<int16_t> c(8, 9, t24));
  REFUSED(gpu::ChannelPower<int16_t> c(8, 4, std::vector<double>()));
  REFUSED(gpu::ChannelPower<int16_t> c(2, 1, std::vector<double>(129, 0.1)));
  REFUSED(gpu::ChannelPower<float> c(8, 4, bad));
  REFUSED(gpu::ChannelPower<int16_t> c(8, 4, huge));
  REFUSED(gpu::ChannelPower<int16_t> c(8, 4, t24, 0.0));
  REFUSED(gpu::ChannelPower<int16_t> c(8, 4, t24, -0.5));
  REFUSED(gpu::ChannelPower<int16_t> c(8, 4, t24, 1.0000001));
  REFUSED(gpu::ChannelPower<float> c(8, 4, t24, std::nan("")));
  gpu::ChannelPower<int16_t> ok(8, 4, t24, 1.0);
  REFUSED(ok.setThresholds(1.0, 2.0));
  REFUSED(ok.setThresholds(1.0, -1.0));
  REFUSED(ok.setThresholds(std::nan(""), 0.0));
  REFUSED(ok.setThresholds(std::vector<double>(7, 1.0), std::vector<double>(7, 0.5)));
  REFUSED(ok.setAlpha(0.0));
  REFUSED(ok.setTaps(std::vector<double>(23, 0.1)));
#undef REFUSED
  // what the rules admit constructs, and answers, without a device
  if (refused([&] {
        gpu::ChannelPower<int16_t> a(8, 4, t24), b(4096, 4096, std::vector<double>(5, 0.2), 1e-9);
        gpu::ChannelPower<float> c(1000, 1, t24, 0.5);
        a.setThresholds(HUGE_VAL, 0.0);
        a.setThresholds(3.0, 3.0);
        a.setAlpha(1.0);
        a.setTaps(t24);
      })) {
    printf("FAIL rules: a valid node was refused\n");
    failures++;
  }
  if (ok.channels() != 8 || !ok.occupied().empty() || ok.levels() != std::vector<double>(8, 0.0) || ok.open() != std::vector<bool>(8, false) ||
      ok.consumed() != 0 || ok.calls() != 0 || ok.sums().size() != 8) {
    printf("FAIL rules: the answers before config()\n");
    failures++;
  }
  printf("rules: %d refused\n", n);
  return failures;
}

static bool within(const std::vector<double> &got, const double *want, size_t M, const char *what, size_t buf) {
  double worst = 0, scale = 0;
  for (size_t k = 0; k < M; k++) { worst = std::max(worst, std::fabs(got[k] - want[k])); scale = std::max(scale, std::fabs(want[k])); }
  printf("graph buffer %zu: max |%s - want| / max want = %.3g\n", buf, what, worst / scale);
  return worst <= 1e-5 * scale;
}

static int runGraph(const char *casePath, const char *tapsPath, const char *xPath, const char *wantPath) {
  std::ifstream f(casePath);
  size_t M = 0, D = 0, nTaps = 0, lens[2] = {0, 0};
  double alpha = 0, openThr = 0, closeThr = 0;
  f >> M >> D >> nTaps >> alpha >> openThr >> closeThr >> lens[0] >> lens[1];
  std::vector<int> occ[2];
  for (int b = 0; b < 2; b++) {
    size_t c = 0;
    f >> c;
    occ[b].resize(c);
    for (size_t i = 0; i < c; i++) f >> occ[b][i];
  }
  if (!f) { fprintf(stderr, "%s: bad case file\n", casePath); return 1; }
  const std::vector<double> taps = readBin<double>(tapsPath, nTaps);
  std::vector<cs> x = readBin<cs>(xPath, lens[0] + lens[1]);
  const std::vector<double> want = readBin<double>(wantPath, 4 * M);
  const size_t bs = std::max(lens[0], lens[1]);

  int failures = 0;
  Feeder<cs> src;
  gpu::ChannelPower<int16_t> node(M, D, taps, alpha);
  node.setThresholds(openThr, closeThr);          // before config(): they hold over it
  src.connect(&node, true);
  src.configure(48000.0, bs);
  std::vector<double> sums[2], levels[2];
  size_t off = 0;
  for (size_t b = 0; b < 2; b++) {
    src.feed(x.data() + off, lens[b]);
    const size_t count = (off + lens[b]) / D - off / D;
    off += lens[b];
    sums[b] = node.sums();
    levels[b] = node.levels();
    if (node.lastCount() != count) { printf("FAIL graph buffer %zu: %zu outputs, want %zu\n", b, node.lastCount(), count); failures++; }
    if (!within(sums[b], &want[(2 * b) * M], M, "sum", b)) { printf("FAIL graph buffer %zu: sums above 1e-5\n", b); failures++; }
    if (!within(levels[b], &want[(2 * b + 1) * M], M, "level", b)) { printf("FAIL graph buffer %zu: levels above 1e-5\n", b); failures++; }
    if (node.occupied() != occ[b]) { printf("FAIL graph buffer %zu: occupied() has %zu channels, want %zu\n", b, node.occupied().size(), occ[b].size()); failures++; }
    const std::vector<bool> open = node.open();
    for (size_t k = 0; k < M; k++)
      if (open[k] != (std::find(occ[b].begin(), occ[b].end(), int(k)) != occ[b].end())) { printf("FAIL graph buffer %zu: open[%zu]\n", b, k); failures++; }
  }
  if (node.consumed() != lens[0] + lens[1] || node.calls() != 2) { printf("FAIL graph: consumed %llu, calls %llu\n", (unsigned long long)node.consumed(), (unsigned long long)node.calls()); failures++; }
  printf("graph: %zu channels, occupied %zu then %zu\n", M, occ[0].size(), occ[1].size());

  // reset: levels, flags and counts go, thresholds stay; the same buffers again give the same bits
  node.reset();
  if (node.consumed() != 0 || node.calls() != 0 || !node.occupied().empty() || node.levels() != std::vector<double>(M, 0.0)) {
    printf("FAIL reset: state left\n");
    failures++;
  }
  off = 0;
  for (size_t b = 0; b < 2; b++) {
    src.feed(x.data() + off, lens[b]);
    off += lens[b];
    const std::vector<double> l = node.levels();
    if (memcmp(node.sums().data(), sums[b].data(), M * sizeof(double)) || memcmp(l.data(), levels[b].data(), M * sizeof(double)) || node.occupied() != occ[b]) {
      printf("FAIL reset: buffer %zu differs from the first run\n", b);
      failures++;
    }
  }
  printf("reset: 2 buffers again\n");

  // the state alone through processDev, on a node of its own
  Feeder<cs> src2;
  gpu::ChannelPower<int16_t> dev(M, D, taps, alpha);
  src2.connect(&dev, true);
  src2.configure(48000.0, bs);
  dev.setThresholds(openThr, closeThr);           // behind config(): they reach the plan
  sdrhip_ctx *ctx = dev.context();
  void *din = 0;
  if (sdrhip_malloc(ctx, bs * sizeof(cs), &din)) return failures + 1;
  off = 0;
  for (size_t b = 0; b < 2; b++) {
    size_t got = 0;
    sdrhip_memcpy_h2d(ctx, din, x.data() + off, lens[b] * sizeof(cs));
    if (!dev.processDev(din, lens[b], 0, &got) || got != (off + lens[b]) / D - off / D) { printf("FAIL processDev: %zu outputs\n", got); failures++; }
    sdrhip_ctx_synchronize(ctx);
    off += lens[b];
    const std::vector<double> l = dev.levels();
    if (memcmp(l.data(), levels[b].data(), M * sizeof(double)) || dev.occupied() != occ[b]) { printf("FAIL processDev: buffer %zu, another state\n", b); failures++; }
  }
  sdrhip_free(ctx, din);
  printf("processDev: 2 buffers\n");

  bool threw = false;
  try {   // another input type
    Feeder<cf> fsrc;
    gpu::ChannelPower<int16_t> wrong(M, D, taps);
    fsrc.connect(&wrong, true);
    fsrc.configure(48000.0, 512);
  } catch (ConfigError &) { threw = true; }
  if (!threw) { printf("FAIL config: a complex float input was accepted by ChannelPower<int16_t>\n"); failures++; }
  return failures;
}

int main(int argc, char **argv) {
  return runMain("usage: test_chanpower rules | graph <case.txt> <taps.bin> <x.bin> <want.bin>\n", [&]() -> int {
    if (argc >= 2 && std::string(argv[1]) == "rules") return runRules();
    if (argc >= 6 && std::string(argv[1]) == "graph") return runGraph(argv[2], argv[3], argv[4], argv[5]);
    return -1;
  });
}
