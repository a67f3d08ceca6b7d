// test_synthesis.cc — sdr::gpu::Synthesis (include/sdr/gpu/synthesis.hh).
//   test_synthesis rules
//       host only: the constructor's rules throw ConfigError
//   test_synthesis run <case.txt> <taps.bin> <x.bin> <want.bin>
//       on the GPU: host rows through gpu::Synthesis::process into a Sink, in the rounds the case lists, against the values the
//       Python side wrote from the numpy restatement: max |z - want| / max |want| <= 1e-5; the per-round output counts and the
//       output Config; then the same rows as strided device rows through processDev on a second node, bit for bit the first
//       node's values, with the elements behind the output row untouched.
// case.txt: M D n_taps n rows  channel...  nrounds len...      taps.bin: n_taps doubles; x.bin: rows x n x (float re, im);
// want.bin: n D x (double re, im)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "sdr/gpu/synthesis.hh"
#include "harness.hh"

typedef std::complex<float> cf;

static int runRules() {
  int failures = 0, n = 0;
  const std::vector<double> t24(24, 0.04);
  std::vector<double> bad = t24;
  bad[7] = HUGE_VAL;
  std::vector<double> huge = t24;
  huge[7] = 1e39;   // finite as a double, not as a float
#define REFUSED(...) do { n++; if (!refused([&] { __VA_ARGS__; })) { printf("FAIL rules: accepted: %s\n", #__VA_ARGS__); failures++; } } while (0)
  REFUSED(gpu::Synthesis s(1, 1, t24));
  REFUSED(gpu::Synthesis s(4097, 8, t24));
  REFUSED(gpu::Synthesis s(17, 8, t24));
  REFUSED(gpu::Synthesis s(38, 8, t24));
  REFUSED(gpu::Synthesis s(8, 0, t24));
  REFUSED(gpu::Synthesis s(8, 9, t24));
  REFUSED(gpu::Synthesis s(8, 4, std::vector<double>()));
  REFUSED(gpu::Synthesis s(8, 2, std::vector<double>(129, 0.1)));
  REFUSED(gpu::Synthesis s(4096, 1, std::vector<double>(65, 0.1)));   // 64 D, not 64 M
  REFUSED(gpu::Synthesis s(8, 4, bad));
  REFUSED(gpu::Synthesis s(8, 4, huge));
  REFUSED(gpu::Synthesis s(8, 4, t24, std::vector<int>(1, 8)));
  REFUSED(gpu::Synthesis s(8, 4, t24, std::vector<int>(1, -1)));
  REFUSED(gpu::Synthesis s(8, 4, t24, std::vector<int>(2, 3)));
#undef REFUSED
  // what the rules admit constructs without a device
  if (refused([&] { gpu::Synthesis a(8, 4, t24), b(4096, 4096, std::vector<double>(5, 0.2)), c(1000, 1, t24, std::vector<int>(1, 999)), d(8, 2, std::vector<double>(128, 0.1)); })) {
    printf("FAIL rules: a valid node was refused\n");
    failures++;
  }
  gpu::Synthesis all(12, 6, t24);
  if (all.rows() != 12 || all.channel(11) != 11 || all.context() != 0 || all.consumed() != 0) { printf("FAIL rules: the default selection\n"); failures++; }
  if (all.process(0, 4)) { printf("FAIL rules: a round was taken before config()\n"); failures++; }
  printf("rules: %d constructions refused\n", n);
  return failures;
}

static int runCase(const char *casePath, const char *tapsPath, const char *xPath, const char *wantPath) {
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
  const std::vector<cf> x = readBin<cf>(xPath, rows * n);
  const size_t no = n * D;
  const std::vector<double> want = readBin<double>(wantPath, no * 2);
  size_t bs = 0;
  for (size_t i = 0; i < nbuf; i++) bs = std::max(bs, lens[i]);

  int failures = 0;
  gpu::Synthesis node(M, D, taps, sel);
  Capture<cf> out;
  node.connect(&out, true);
  const double Fs = 6000.0;
  node.config(Fs, bs);
  if (out.cfg.type() != Config::typeId<cf>() || out.cfg.sampleRate() != Fs * double(D) || out.cfg.bufferSize() != bs * D) {
    printf("FAIL run: output config (rate %g, buffer %zu)\n", out.cfg.sampleRate(), out.cfg.bufferSize());
    failures++;
  }
  size_t off = 0;
  for (size_t b = 0; b < nbuf; b++) {
    const size_t before = out.data.size();
    if (!node.process(x.data() + off, lens[b], n)) { printf("FAIL run round %zu: dropped\n", b); failures++; }
    off += lens[b];
    if (out.data.size() - before != lens[b] * D) { printf("FAIL run round %zu: %zu outputs, want %zu\n", b, out.data.size() - before, lens[b] * D); failures++; }
  }
  if (node.process(x.data(), bs + 1, n)) { printf("FAIL run: a round above the configured columns was taken\n"); failures++; }
  if (node.consumed() != n) { printf("FAIL run: consumed %llu\n", (unsigned long long)node.consumed()); failures++; }
  if (out.data.size() != no) { printf("FAIL run: %zu outputs in all, want %zu\n", out.data.size(), no); return failures + 1; }
  double worst = 0, scale = 0;
  for (size_t j = 0; j < no; j++) {
    worst = std::max(worst, std::hypot(double(out.data[j].real()) - want[2 * j], double(out.data[j].imag()) - want[2 * j + 1]));
    scale = std::max(scale, std::hypot(want[2 * j], want[2 * j + 1]));
  }
  printf("run: %zu rows x %zu columns, max |z - want| / max |want| = %.3g\n", rows, n, worst / scale);
  if (!(worst <= 1e-5 * scale)) { printf("FAIL run: above 1e-5\n"); failures++; }

  // the same rows as strided device rows, one call, on a node of its own
  gpu::Synthesis dev(M, D, taps, sel);
  dev.config(Fs, n);
  sdrhip_ctx *ctx = dev.context();
  const size_t stride = n + 5, tail = 9;
  std::vector<cf> hin(rows * stride, cf(3.f, 3.f)), hout(no + tail, cf(7.f, 7.f));
  for (size_t i = 0; i < rows; i++) memcpy(&hin[i * stride], &x[i * n], n * sizeof(cf));
  void *din = 0, *dout = 0;
  if (sdrhip_malloc(ctx, hin.size() * sizeof(cf), &din) || sdrhip_malloc(ctx, hout.size() * sizeof(cf), &dout)) return failures + 1;
  sdrhip_memcpy_h2d(ctx, din, hin.data(), hin.size() * sizeof(cf));
  sdrhip_memcpy_h2d(ctx, dout, hout.data(), hout.size() * sizeof(cf));
  size_t got = 0;
  if (!dev.processDev(din, n, stride, dout, &got) || got != no) { printf("FAIL processDev: %zu outputs\n", got); failures++; }
  sdrhip_ctx_synchronize(ctx);
  sdrhip_memcpy_d2h(ctx, hout.data(), dout, hout.size() * sizeof(cf));
  if (memcmp(hout.data(), out.data.data(), no * sizeof(cf))) { printf("FAIL processDev differs from the host rounds'\n"); failures++; }
  for (size_t j = no; j < no + tail; j++)
    if (hout[j] != cf(7.f, 7.f)) { printf("FAIL processDev: element %zu behind the count was written\n", j); failures++; break; }
  sdrhip_free(ctx, din); sdrhip_free(ctx, dout);
  dev.reset();
  if (dev.consumed() != 0) { printf("FAIL reset: consumed %llu\n", (unsigned long long)dev.consumed()); failures++; }
  printf("processDev: %zu rows\n", rows);
  return failures;
}

int main(int argc, char **argv) {
  return runMain("usage: test_synthesis rules | run <case.txt> <taps.bin> <x.bin> <want.bin>\n", [&]() -> int {
    if (argc >= 2 && std::string(argv[1]) == "rules") return runRules();
    if (argc >= 6 && std::string(argv[1]) == "run") return runCase(argv[2], argv[3], argv[4], argv[5]);
    return -1;
  });
}
