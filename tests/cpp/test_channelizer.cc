// test_channelizer.cc — sdr::gpu::Channelizer<Scalar> (include/sdr/gpu/channelizer.hh).
//   test_channelizer rules
//       host only: the constructor's rules throw ConfigError
//   test_channelizer graph <case.txt> <taps.bin> <x.bin> <want.bin>
//       on the GPU: a cs16 stream through Source -> gpu::Channelizer<int16_t> -> one Sink per selected row, in the buffers the
//       case lists, against the values the Python side wrote from the numpy restatement: max |y - want| / max |want| <= 1e-5
//       over all rows; the per-buffer output counts and the output Config; then the same stream as device rows through
//       processDev on a second node, bit for bit the graph's values; and the config rule for another input type.
// case.txt: M D n_taps n rows  channel...  nbuf len...      taps.bin: n_taps doubles; x.bin: n x (int16 re, im);
// want.bin: rows x (n / D) x (double re, im)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "sdr/gpu/channelizer.hh"
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
  REFUSED(gpu::Channelizer<int16_t> c(1, 1, t24));
  REFUSED(gpu::Channelizer<int16_t> c(4097, 8, t24));
  REFUSED(gpu::Channelizer<int16_t> c(17, 8, t24));
  REFUSED(gpu::Channelizer<float> c(38, 8, t24));
  REFUSED(gpu::Channelizer<int16_t> c(8, 0, t24));
  REFUSED(gpu::Channelizer<int16_t> c(8, 9, t24));
  REFUSED(gpu::Channelizer<int16_t> c(8, 4, std::vector<double>()));
  REFUSED(gpu::Channelizer<int16_t> c(2, 1, std::vector<double>(129, 0.1)));
  REFUSED(gpu::Channelizer<float> c(8, 4, bad));
  REFUSED(gpu::Channelizer<int16_t> c(8, 4, huge));
  REFUSED(gpu::Channelizer<int16_t> c(8, 4, t24, std::vector<int>(1, 8)));
  REFUSED(gpu::Channelizer<int16_t> c(8, 4, t24, std::vector<int>(1, -1)));
  REFUSED(gpu::Channelizer<int16_t> c(8, 4, t24, std::vector<int>(2, 3)));
#undef REFUSED
  // what the rules admit constructs without a device
  if (refused([&] { gpu::Channelizer<int16_t> a(8, 4, t24), b(4096, 4096, std::vector<double>(5, 0.2)), c(1000, 1, t24, std::vector<int>(1, 999)); })) {
    printf("FAIL rules: a valid node was refused\n");
    failures++;
  }
  gpu::Channelizer<float> all(12, 6, t24);
  if (all.rows() != 12 || all.channel(11) != 11 || all.source(11) == 0) { printf("FAIL rules: the default selection\n"); failures++; }
  printf("rules: %d constructions refused\n", n);
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
  gpu::Channelizer<int16_t> node(M, D, taps, sel);
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
  gpu::Channelizer<int16_t> dev(M, D, taps, sel);
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

  bool threw = false;
  try {   // another input type
    Feeder<cf> fsrc;
    gpu::Channelizer<int16_t> wrong(M, D, taps);
    fsrc.connect(&wrong, true);
    fsrc.configure(Fs, 512);
  } catch (ConfigError &) { threw = true; }
  if (!threw) { printf("FAIL config: a complex float input was accepted by Channelizer<int16_t>\n"); failures++; }
  return failures;
}

int main(int argc, char **argv) {
  return runMain("usage: test_channelizer rules | graph <case.txt> <taps.bin> <x.bin> <want.bin>\n", [&]() -> int {
    if (argc >= 2 && std::string(argv[1]) == "rules") return runRules();
    if (argc >= 6 && std::string(argv[1]) == "graph") return runGraph(argv[2], argv[3], argv[4], argv[5]);
    return -1;
  });
}
