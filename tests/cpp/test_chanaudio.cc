// test_chanaudio.cc — sdr::gpu::AudioChannelizer<Scalar> (include/sdr/gpu/chanaudio.hh).
//   test_chanaudio rules
//       host only: the constructor's rules throw ConfigError
//   test_chanaudio graph <case.txt> <taps.bin> <x.bin> <want.bin>
//       on the GPU: a cs16 stream through Source -> gpu::AudioChannelizer<int16_t> -> one Sink per selected row, in the buffers
//       the case lists, bit for bit the int16 rows the Python side wrote (its wrapper's, fed the same buffers: the FM rows follow
//       the per-call convention); the per-buffer output counts and the output Config; then the same buffers as device rows
//       through processDev on a second node; and the config rule for another input type.
// case.txt: M D n_taps n rows  (channel mode)...  nbuf len...   (row i's gain is 0.5 + i)      taps.bin: n_taps doubles;
// x.bin: n x (int16 re, im); want.bin: rows x (n / D) int16
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "sdr/gpu/chanaudio.hh"
#include "harness.hh"

typedef std::complex<int16_t> cs;
typedef std::complex<float> cf;

static int runRules() {
  int failures = 0, n = 0;
  const std::vector<double> t24(24, 0.04);
  std::vector<double> bad = t24;
  bad[7] = HUGE_VAL;
  const std::vector<int> two(2, 3), none;
  std::vector<int> sel3;
  sel3.push_back(5); sel3.push_back(0); sel3.push_back(2);
  std::vector<int> m3(3, int(SDRHIP_EPI_AM));
  std::vector<float> g3(3, 2.0f);
#define REFUSED(...) do { n++; if (!refused([&] { __VA_ARGS__; })) { printf("FAIL rules: accepted: %s\n", #__VA_ARGS__); failures++; } } while (0)
  // the channelizer's
  REFUSED(gpu::AudioChannelizer<int16_t> c(1, 1, t24));
  REFUSED(gpu::AudioChannelizer<int16_t> c(4097, 8, t24));
  REFUSED(gpu::AudioChannelizer<int16_t> c(17, 8, t24));
  REFUSED(gpu::AudioChannelizer<int16_t> c(8, 0, t24));
  REFUSED(gpu::AudioChannelizer<int16_t> c(8, 9, t24));
  REFUSED(gpu::AudioChannelizer<int16_t> c(8, 4, std::vector<double>()));
  REFUSED(gpu::AudioChannelizer<float> c(8, 4, bad));
  REFUSED(gpu::AudioChannelizer<int16_t> c(8, 4, t24, std::vector<int>(1, 8)));
  REFUSED(gpu::AudioChannelizer<int16_t> c(8, 4, t24, two));
  // modes and gains: one per row, a demodulator, finite
  REFUSED(gpu::AudioChannelizer<int16_t> c(8, 4, t24, sel3, std::vector<int>(2, int(SDRHIP_EPI_FM))));
  REFUSED(gpu::AudioChannelizer<int16_t> c(8, 4, t24, sel3, std::vector<int>(3, int(SDRHIP_EPI_NONE))));
  REFUSED(gpu::AudioChannelizer<int16_t> c(8, 4, t24, sel3, std::vector<int>(3, 4)));
  REFUSED(gpu::AudioChannelizer<int16_t> c(8, 4, t24, sel3, m3, std::vector<float>(4, 1.0f)));
  REFUSED(gpu::AudioChannelizer<float> c(8, 4, t24, sel3, m3, std::vector<float>(3, INFINITY)));
  REFUSED(gpu::AudioChannelizer<float> c(8, 4, t24, none, none, std::vector<float>(8, NAN)));
#undef REFUSED
  // what the rules admit constructs without a device
  if (refused([&] { gpu::AudioChannelizer<int16_t> a(8, 4, t24), b(4096, 4096, std::vector<double>(5, 0.2)), c(8, 4, t24, sel3, m3, g3); })) {
    printf("FAIL rules: a valid node was refused\n");
    failures++;
  }
  gpu::AudioChannelizer<float> all(12, 6, t24);
  if (all.rows() != 12 || all.channel(11) != 11 || all.source(11) == 0 || all.mode(3) != SDRHIP_EPI_FM || all.gain(3) != 1.0f) {
    printf("FAIL rules: the defaults\n");
    failures++;
  }
  gpu::AudioChannelizer<int16_t> some(8, 4, t24, sel3, m3, g3);
  some.setMode(1, SDRHIP_EPI_USB);   // before config(): noted
  some.setGain(2, 0.25f);
  if (some.rows() != 3 || some.mode(0) != SDRHIP_EPI_AM || some.mode(1) != SDRHIP_EPI_USB || some.gain(2) != 0.25f || some.consumed() != 0) {
    printf("FAIL rules: the rows' settings\n");
    failures++;
  }
  printf("rules: %d constructions refused\n", n);
  return failures;
}

static int runGraph(const char *casePath, const char *tapsPath, const char *xPath, const char *wantPath) {
  std::ifstream f(casePath);
  size_t M = 0, D = 0, nTaps = 0, n = 0, rows = 0, nbuf = 0;
  f >> M >> D >> nTaps >> n >> rows;
  std::vector<int> sel(rows), modes(rows);
  std::vector<float> gains(rows);
  for (size_t i = 0; i < rows; i++) { f >> sel[i] >> modes[i]; gains[i] = 0.5f + float(i); }
  f >> nbuf;
  std::vector<size_t> lens(nbuf);
  for (size_t i = 0; i < nbuf; i++) f >> lens[i];
  if (!f) { fprintf(stderr, "%s: bad case file\n", casePath); return 1; }
  const std::vector<double> taps = readBin<double>(tapsPath, nTaps);
  std::vector<cs> x = readBin<cs>(xPath, n);
  const size_t no = n / D;
  const std::vector<int16_t> want = readBin<int16_t>(wantPath, rows * no);
  size_t bs = 0;
  for (size_t i = 0; i < nbuf; i++) bs = std::max(bs, lens[i]);

  int failures = 0;
  Feeder<cs> src;
  gpu::AudioChannelizer<int16_t> node(M, D, taps, sel, modes, gains);
  std::vector< Capture<int16_t> > outs(rows);
  src.connect(&node, true);
  for (size_t i = 0; i < rows; i++) node.source(i)->connect(&outs[i], true);
  const double Fs = 48000.0;
  src.configure(Fs, bs);
  const size_t stride = (bs + D - 1) / D;
  for (size_t i = 0; i < rows; i++)
    if (outs[i].cfg.type() != Config::typeId<int16_t>() || outs[i].cfg.sampleRate() != Fs / double(D) || outs[i].cfg.bufferSize() != stride) {
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
  for (size_t i = 0; i < rows; i++) {
    if (outs[i].data.size() != no) { printf("FAIL graph row %zu: %zu outputs in all, want %zu\n", i, outs[i].data.size(), no); return failures + 1; }
    if (memcmp(outs[i].data.data(), &want[i * no], no * sizeof(int16_t))) { printf("FAIL graph row %zu (mode %d) differs from the Python side's\n", i, modes[i]); failures++; }
  }
  printf("graph: %zu rows x %zu outputs\n", rows, no);

  // the same buffers as device rows on a node of its own
  Feeder<cs> src2;
  gpu::AudioChannelizer<int16_t> dev(M, D, taps, sel, modes, gains);
  src2.connect(&dev, true);
  src2.configure(Fs, bs);
  sdrhip_ctx *ctx = dev.context();
  const size_t dstride = stride + 5;
  std::vector<int16_t> host(rows * dstride);
  void *din = 0, *dout = 0;
  if (sdrhip_malloc(ctx, bs * sizeof(cs), &din) || sdrhip_malloc(ctx, host.size() * sizeof(int16_t), &dout)) return failures + 1;
  off = 0;
  size_t at = 0;
  for (size_t b = 0; b < nbuf; b++) {
    if (!lens[b]) continue;
    host.assign(host.size(), int16_t(7777));
    sdrhip_memcpy_h2d(ctx, din, x.data() + off, lens[b] * sizeof(cs));
    sdrhip_memcpy_h2d(ctx, dout, host.data(), host.size() * sizeof(int16_t));
    const size_t count = (off + lens[b]) / D - off / D;
    size_t got = 0;
    if (!dev.processDev(din, lens[b], dout, dstride, &got) || got != count) { printf("FAIL processDev buffer %zu: %zu outputs\n", b, got); failures++; }
    sdrhip_ctx_synchronize(ctx);
    sdrhip_memcpy_d2h(ctx, host.data(), dout, host.size() * sizeof(int16_t));
    for (size_t i = 0; i < rows; i++) {
      if (memcmp(&host[i * dstride], &want[i * no + at], count * sizeof(int16_t))) { printf("FAIL processDev buffer %zu row %zu differs\n", b, i); failures++; }
      for (size_t j = count; j < dstride; j++)
        if (host[i * dstride + j] != 7777) { printf("FAIL processDev row %zu: element %zu behind the count was written\n", i, j); failures++; break; }
    }
    off += lens[b];
    at += count;
  }
  sdrhip_free(ctx, din); sdrhip_free(ctx, dout);
  printf("processDev: %zu rows\n", rows);

  bool threw = false;
  try {   // another input type
    Feeder<cf> fsrc;
    gpu::AudioChannelizer<int16_t> wrong(M, D, taps);
    fsrc.connect(&wrong, true);
    fsrc.configure(Fs, 512);
  } catch (ConfigError &) { threw = true; }
  if (!threw) { printf("FAIL config: a complex float input was accepted by AudioChannelizer<int16_t>\n"); failures++; }
  return failures;
}

int main(int argc, char **argv) {
  return runMain("usage: test_chanaudio rules | graph <case.txt> <taps.bin> <x.bin> <want.bin>\n", [&]() -> int {
    if (argc >= 2 && std::string(argv[1]) == "rules") return runRules();
    if (argc >= 6 && std::string(argv[1]) == "graph") return runGraph(argv[2], argv[3], argv[4], argv[5]);
    return -1;
  });
}
