// test_resample.cc — sdr::gpu::InpolSubSampler<iScalar, oScalar> and gpu::InpolSubSamplerBank (include/sdr/gpu/resample.hh).
//   test_resample rules
//       host only: the constructor's frac rule
//   test_resample nodes <cases.txt> <golden dir> <table.bin>
//       on the GPU: every g22_inpol_* stream through Source -> gpu::InpolSubSampler -> Sink in its recorded buffers, with the
//       reference's table, against the reference's outputs, per-buffer counts and final mu; the config rules; then the 256-sample
//       buffer of the streams of a type as the rows of one InpolSubSamplerBank (a frac per row) after the buffers before it,
//       through host pointers and as strided device rows.
// cases.txt, one stream per line: name dtype frac_bits count outputs  nlens lens...  counts...  mu_bits...
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "sdr/gpu/resample.hh"
#include "harness.hh"

struct Case {
  std::string name, dtype;
  float frac;
  size_t count, outputs;
  std::vector<size_t> lens, counts;
  std::vector<uint32_t> mu;
};

static uint32_t bitsOf(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

static int runRules() {
  int failures = 0;
  const float bad[] = {0.f, -1.f, 0.12f, 4097.f};
  for (size_t i = 0; i < 4; i++) {
    bool threw = false;
    try { gpu::InpolSubSampler<float> node(bad[i]); } catch (ConfigError &) { threw = true; } catch (SDRError &) {}
    if (!threw) { printf("FAIL rules: frac %g was accepted\n", (double)bad[i]); failures++; }
  }
  printf("rules: 4 fractions refused\n");
  return failures;
}

template <class I, class O>
static int runNode(const Case &k, const std::string &dir, const std::vector<float> &table) {
  std::vector<I> x = readBin<I>(dir + "/g22_inpol_" + k.dtype + "_x.bin", k.count);
  std::vector<O> want = readBin<O>(dir + "/" + k.name + "_y.bin", k.outputs);
  Feeder<I> src;
  gpu::InpolSubSampler<I, O> node(k.frac, table.data());
  Capture<O> out;
  src.connect(&node, true); node.connect(&out, true);
  src.configure(8000.0, 1000);
  int failures = 0;
  const size_t cap = (size_t)(1001.0 / (double)k.frac) + 2;
  if (out.cfg.type() != Config::typeId<O>() || out.cfg.sampleRate() != 8000.0 / k.frac || out.cfg.bufferSize() != cap) {
    printf("FAIL %s: output config (rate %g, buffer %zu, want %g, %zu)\n", k.name.c_str(), out.cfg.sampleRate(), out.cfg.bufferSize(),
           8000.0 / k.frac, cap);
    failures++;
  }
  size_t off = 0;
  for (size_t b = 0; b < k.lens.size(); b++) {
    const size_t before = out.data.size();
    src.feed(x.data() + off, k.lens[b]);
    off += k.lens[b];
    if (out.data.size() - before != k.counts[b]) {
      printf("FAIL %s buffer %zu: %zu outputs, want %zu\n", k.name.c_str(), b, out.data.size() - before, k.counts[b]);
      failures++;
    }
  }
  if (out.data.size() != want.size() || memcmp(out.data.data(), want.data(), want.size() * sizeof(O))) {
    printf("FAIL %s: the outputs differ from the reference's\n", k.name.c_str());
    failures++;
  }
  if (bitsOf(node.mu()) != k.mu.back()) { printf("FAIL %s: mu %g\n", k.name.c_str(), (double)node.mu()); failures++; }
  return failures;
}

template <class I, class O>
static int configRules() {
  int failures = 0;
  bool threw = false;
  try {   // another input type
    Feeder<double> src;
    gpu::InpolSubSampler<I, O> node(2.0f);
    src.connect(&node, true);
    src.configure(8000.0, 512);
  } catch (ConfigError &) { threw = true; }
  if (!threw) { printf("FAIL config: a double input was accepted\n"); failures++; }
  return failures;
}

// the streams of one type as the rows of one bank, a frac per row: the buffers before the 256-sample one through host pointers
// (both banks), then that buffer through host pointers and as strided device rows
template <class I, class O>
static int runBank(const std::vector<Case> &cases, const char *dtype, const std::string &dir, const std::vector<float> &table) {
  std::vector<const Case *> rows;
  for (size_t i = 0; i < cases.size(); i++) if (cases[i].dtype == dtype) rows.push_back(&cases[i]);
  if (rows.empty()) return 0;
  const size_t C = rows.size(), stride = 256 + 8;
  const std::vector<size_t> &lens = rows[0]->lens;
  size_t b256 = 0, off = 0;
  while (b256 < lens.size() && lens[b256] != 256) off += lens[b256++];
  if (b256 == lens.size()) { printf("FAIL bank %s: no 256-sample buffer\n", dtype); return 1; }
  std::vector<I> all = readBin<I>(dir + "/g22_inpol_" + dtype + "_x.bin", rows[0]->count);
  std::vector<float> frac(C);
  for (size_t c = 0; c < C; c++) frac[c] = rows[c]->frac;
  int failures = 0;
  gpu::InpolSubSamplerBank<I, O> host(frac, 256, table.data()), dev(frac, 256, table.data());
  const size_t cap = host.outCapacity(256), ostride = cap + 5;
  std::vector<I> x(C * stride);
  std::vector<O> out(C * ostride, O(9)), dout_h(C * ostride, O(7));
  std::vector<uint32_t> counts(C, 99), dcounts(C, 98);
  std::vector<size_t> skip(C, 0);   // the outputs of the buffers before
  size_t at = 0;
  for (size_t b = 0; b < b256; b++) {
    for (size_t c = 0; c < C; c++) std::copy(all.begin() + at, all.begin() + at + lens[b], x.begin() + c * stride);
    if (!host.process(x.data(), lens[b], stride, out.data(), ostride, counts.data()) ||
        !dev.process(x.data(), lens[b], stride, dout_h.data(), ostride, dcounts.data())) { printf("FAIL bank %s: process\n", dtype); return 1; }
    for (size_t c = 0; c < C; c++) {
      if (counts[c] != rows[c]->counts[b] || dcounts[c] != counts[c]) { printf("FAIL bank %s row %zu buffer %zu: count %u\n", dtype, c, b, counts[c]); failures++; }
      skip[c] += counts[c];
    }
    at += lens[b];
  }
  for (size_t c = 0; c < C; c++) std::copy(all.begin() + off, all.begin() + off + 256, x.begin() + c * stride);
  std::fill(out.begin(), out.end(), O(9));
  std::fill(dout_h.begin(), dout_h.end(), O(7));
  if (!host.process(x.data(), 256, stride, out.data(), ostride, counts.data())) { printf("FAIL bank %s: process\n", dtype); return 1; }
  void *din = 0, *dout = 0, *dcnt = 0;
  sdrhip_ctx *ctx = dev.context();
  if (sdrhip_malloc(ctx, x.size() * sizeof(I), &din) || sdrhip_malloc(ctx, dout_h.size() * sizeof(O), &dout) || sdrhip_malloc(ctx, C * 4, &dcnt)) return 1;
  sdrhip_memcpy_h2d(ctx, din, x.data(), x.size() * sizeof(I));
  sdrhip_memcpy_h2d(ctx, dout, dout_h.data(), dout_h.size() * sizeof(O));
  if (!dev.processDev(din, 256, stride, dout, ostride, static_cast<uint32_t *>(dcnt))) { printf("FAIL bank %s: processDev\n", dtype); failures++; }
  sdrhip_ctx_synchronize(ctx);
  sdrhip_memcpy_d2h(ctx, dout_h.data(), dout, dout_h.size() * sizeof(O));
  sdrhip_memcpy_d2h(ctx, dcounts.data(), dcnt, C * 4);
  std::vector<float> mu;
  std::vector<O> line;
  dev.state(mu, line);
  for (size_t c = 0; c < C; c++) {
    std::vector<O> want = readBin<O>(dir + "/" + rows[c]->name + "_y.bin", rows[c]->outputs);
    if (counts[c] != rows[c]->counts[b256] || dcounts[c] != counts[c]) {
      printf("FAIL bank %s row %zu: counts %u / %u, want %zu\n", dtype, c, counts[c], dcounts[c], rows[c]->counts[b256]);
      failures++;
      continue;
    }
    if (memcmp(&out[c * ostride], &want[skip[c]], counts[c] * sizeof(O)) || memcmp(&dout_h[c * ostride], &want[skip[c]], counts[c] * sizeof(O))) {
      printf("FAIL bank %s row %zu: outputs\n", dtype, c);
      failures++;
    }
    for (size_t i = cap; i < ostride; i++)   // behind the capacity a row is the caller's
      if (out[c * ostride + i] != O(9) || dout_h[c * ostride + i] != O(7)) { printf("FAIL bank %s row %zu: element %zu behind the capacity was written\n", dtype, c, i); failures++; break; }
    for (size_t i = counts[c]; i < cap; i++)   // behind its count a device row is left alone
      if (dout_h[c * ostride + i] != O(7)) { printf("FAIL bank %s row %zu: element %zu behind the count was written\n", dtype, c, i); failures++; break; }
    if (bitsOf(mu[c]) != rows[c]->mu[b256]) { printf("FAIL bank %s row %zu: mu %g\n", dtype, c, (double)mu[c]); failures++; }
    if (memcmp(&line[c * 8], &x[c * stride + 248], 8 * sizeof(O)) && sizeof(I) == sizeof(O)) { printf("FAIL bank %s row %zu: line\n", dtype, c); failures++; }
  }
  // a fresh node behind row 0, the others as they are; then every row afresh
  dev.setChannel(0, 3.0f);
  dev.state(mu, line);
  if (mu[0] != 0.f || (C > 1 && bitsOf(mu[1]) != rows[1]->mu[b256])) { printf("FAIL bank %s: setChannel\n", dtype); failures++; }
  dev.reset();
  dev.state(mu, line);
  for (size_t c = 0; c < C; c++) if (mu[c] != 0.f || line[c * 8 + 7] != O(0)) { printf("FAIL bank %s row %zu: reset\n", dtype, c); failures++; }
  sdrhip_free(ctx, din); sdrhip_free(ctx, dout); sdrhip_free(ctx, dcnt);
  printf("bank %s: %zu rows\n", dtype, C);
  return failures;
}

int main(int argc, char **argv) {
  if (argc >= 2 && std::string(argv[1]) == "rules") {
    int failures = 0;
    try { failures = runRules(); } catch (SDRError &e) { printf("FAIL exception: %s\n", e.what()); failures++; }
    printf("%s (%d failures)\n", failures ? "FAILED" : "OK", failures);
    return failures ? 1 : 0;
  }
  if (argc < 5 || std::string(argv[1]) != "nodes") { fprintf(stderr, "usage: test_resample rules | nodes <cases.txt> <golden dir> <table.bin>\n"); return 2; }
  std::vector<Case> cases;
  std::ifstream f(argv[2]);
  std::string line;
  while (std::getline(f, line)) {
    std::istringstream s(line);
    Case k;
    size_t nl = 0;
    uint32_t fb = 0;
    s >> k.name >> k.dtype >> fb >> k.count >> k.outputs >> nl;
    if (!s) continue;
    memcpy(&k.frac, &fb, 4);
    k.lens.resize(nl); k.counts.resize(nl); k.mu.resize(nl);
    for (size_t i = 0; i < nl; i++) s >> k.lens[i];
    for (size_t i = 0; i < nl; i++) s >> k.counts[i];
    for (size_t i = 0; i < nl; i++) s >> k.mu[i];
    cases.push_back(k);
  }
  const std::string dir = argv[3];
  const std::vector<float> table = readBin<float>(argv[4], 129 * 8);
  typedef std::complex<float> cf;
  typedef std::complex<int16_t> cs;
  int failures = 0;
  try {
    for (size_t i = 0; i < cases.size(); i++) {
      const Case &k = cases[i];
      failures += k.dtype == "f32" ? runNode<float, float>(k, dir, table) : k.dtype == "cf32" ? runNode<cf, cf>(k, dir, table)
                  : k.dtype == "i16" ? runNode<int16_t, int16_t>(k, dir, table) : runNode<cs, cf>(k, dir, table);
    }
    printf("nodes: %zu streams\n", cases.size());
    failures += configRules<float, float>() + configRules<cs, cf>();
    failures += runBank<float, float>(cases, "f32", dir, table) + runBank<cf, cf>(cases, "cf32", dir, table);
    failures += runBank<int16_t, int16_t>(cases, "i16", dir, table) + runBank<cs, cf>(cases, "cs16_cf32", dir, table);
  } catch (SDRError &e) {
    printf("FAIL exception: %s\n", e.what());
    failures++;
  }
  printf("%s (%d failures)\n", failures ? "FAILED" : "OK", failures);
  return failures ? 1 : 0;
}
