// test_changroup.cc — sdr::gpu::ChannelGroup<Node> (include/sdr/gpu/changroup.hh).
//   test_changroup rules
//       host only: add() after the first call, a node added twice and a ninth add() throw ConfigError; a call over nodes that
//       were never configured is refused and changes nothing
//   test_changroup gpu
//       on the GPU: a group of two gpu::Channelizer<int16_t> of different shapes, then one of two gpu::RealAudioChannelizer<int16_t>
//       (FM / AM / USB rows, gains), each against the same stream through a second pair of nodes' own processDev — twins, configured
//       alike — over three calls of different lengths per member (one of them empty): rows and consumed(), bit for bit.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "sdr/gpu/chanreal.hh"
#include "sdr/gpu/changroup.hh"
#include "harness.hh"

typedef std::complex<int16_t> cs;
typedef std::complex<float> cf;

static std::vector<double> prototype(size_t M, size_t nTaps) {
  std::vector<double> h(nTaps);
  for (size_t i = 0; i < nTaps; i++) {
    const double t = (double(i) - double(nTaps - 1) / 2) / double(M), w = 0.5 - 0.5 * std::cos(2 * M_PI * double(i + 1) / double(nTaps + 1));
    h[i] = (t == 0 ? 1.0 : std::sin(M_PI * t) / (M_PI * t)) / double(M) * w;
  }
  return h;
}

static int runRules() {
  int failures = 0;
  const std::vector<double> taps = prototype(8, 24);
  gpu::Channelizer<int16_t> a(8, 4, taps), b(12, 6, taps);
  gpu::ChannelGroup< gpu::Channelizer<int16_t> > g;
  g.add(a);
  g.add(b);
  if (g.size() != 2) { printf("FAIL rules: size %zu\n", g.size()); failures++; }
  // never configured: no plan, so the first call is refused — and it was the first call
  const void *in[2] = {0, 0};
  void *out[2] = {0, 0};
  const size_t n[2] = {16, 16}, stride[2] = {0, 0};
  size_t got[2] = {7, 7};
  if (g.processDev(in, n, out, stride, got)) { printf("FAIL rules: a call over unconfigured nodes was accepted\n"); failures++; }
  if (a.consumed() != 0 || b.consumed() != 0) { printf("FAIL rules: a refused call moved a node\n"); failures++; }
  gpu::Channelizer<int16_t> c(8, 4, taps);
  if (!refused([&] { g.add(c); })) { printf("FAIL rules: add() after the first call was accepted\n"); failures++; }
  g.close();
  if (refused([&] { g.add(c); })) { printf("FAIL rules: add() after close() was refused\n"); failures++; }
  if (!refused([&] { g.add(c); })) { printf("FAIL rules: a node was accepted twice\n"); failures++; }
  gpu::ChannelGroup< gpu::Channelizer<int16_t> > full;
  std::vector< gpu::Channelizer<int16_t> * > eight;
  for (int i = 0; i < SDRHIP_CHANGROUP_MAX; i++) { eight.push_back(new gpu::Channelizer<int16_t>(8, 4, taps)); full.add(*eight.back()); }
  if (!refused([&] { full.add(b); })) { printf("FAIL rules: a ninth member was accepted\n"); failures++; }
  for (size_t i = 0; i < eight.size(); i++) delete eight[i];
  printf("rules: 3 adds refused\n");
  return failures;
}

// two members and their twins on streams of their own; Elem: the rows' element
template <class Node, class In, class Elem>
static int runPair(const char *what, Node *nodes[4], const std::vector<In> x[2]) {
  int failures = 0;
  Feeder<In> src[4];
  for (int i = 0; i < 4; i++) {
    src[i].connect(nodes[i], true);
    src[i].configure(48000.0, x[i & 1].size());
  }
  sdrhip_ctx *ctx = nodes[0]->context();
  gpu::ChannelGroup<Node> group;
  group.add(*nodes[0]);
  group.add(*nodes[1]);
  void *din[2] = {0, 0}, *dout[2] = {0, 0}, *dtwin[2] = {0, 0};
  size_t stride[2], rows[2];
  for (int i = 0; i < 2; i++) {
    rows[i] = nodes[i]->rows();
    stride[i] = nodes[i]->outStride() + 3;
    if (sdrhip_malloc(ctx, x[i].size() * sizeof(In), &din[i]) || sdrhip_malloc(ctx, rows[i] * stride[i] * sizeof(Elem), &dout[i]) ||
        sdrhip_malloc(ctx, rows[i] * stride[i] * sizeof(Elem), &dtwin[i]))
      return 1;
  }
  // per call and member: the samples taken (member 1 sits out the second call)
  const size_t third[2] = {x[0].size() / 3, x[1].size() / 3};
  const size_t lens[3][2] = {{third[0] + 1, 5}, {7, 0}, {x[0].size() - third[0] - 8, x[1].size() - 5}};
  size_t off[2] = {0, 0};
  for (int c = 0; c < 3; c++) {
    std::vector<Elem> host[2], twin[2];
    size_t got[2] = {99, 99}, want[2] = {0, 0};
    for (int i = 0; i < 2; i++) {
      host[i].assign(rows[i] * stride[i], Elem(7));
      twin[i] = host[i];
      sdrhip_memcpy_h2d(ctx, din[i], x[i].data() + off[i], lens[c][i] * sizeof(In));
      sdrhip_memcpy_h2d(ctx, dout[i], host[i].data(), host[i].size() * sizeof(Elem));
      sdrhip_memcpy_h2d(ctx, dtwin[i], twin[i].data(), twin[i].size() * sizeof(Elem));
    }
    const void *in[2] = {din[0], din[1]};
    const size_t n[2] = {lens[c][0], lens[c][1]};
    if (!group.processDev(in, n, dout, stride, got)) { printf("FAIL %s call %d: the group call was refused\n", what, c); failures++; }
    for (int i = 0; i < 2; i++)
      if (n[i] && !nodes[2 + i]->processDev(din[i], n[i], dtwin[i], stride[i], &want[i])) { printf("FAIL %s call %d: twin %d refused\n", what, c, i); failures++; }
    sdrhip_ctx_synchronize(ctx);
    for (int i = 0; i < 2; i++) {
      off[i] += n[i];
      sdrhip_memcpy_d2h(ctx, host[i].data(), dout[i], host[i].size() * sizeof(Elem));
      sdrhip_memcpy_d2h(ctx, twin[i].data(), dtwin[i], twin[i].size() * sizeof(Elem));
      if (got[i] != want[i]) { printf("FAIL %s call %d member %d: %zu outputs, the twin %zu\n", what, c, i, got[i], want[i]); failures++; }
      if (memcmp(host[i].data(), twin[i].data(), host[i].size() * sizeof(Elem))) { printf("FAIL %s call %d member %d: rows differ from the twin's\n", what, c, i); failures++; }
      if (nodes[i]->consumed() != nodes[2 + i]->consumed() || nodes[i]->consumed() != off[i]) { printf("FAIL %s call %d member %d: consumed\n", what, c, i); failures++; }
    }
    if (c == 2 && (got[0] == 0 || got[1] == 0)) { printf("FAIL %s: the last call wrote nothing\n", what); failures++; }
  }
  group.close();
  for (int i = 0; i < 2; i++) { sdrhip_free(ctx, din[i]); sdrhip_free(ctx, dout[i]); sdrhip_free(ctx, dtwin[i]); }
  printf("%s: 3 group calls of 2 members equal the twins'\n", what);
  return failures;
}

static int runGpu() {
  int failures = 0;
  uint32_t seed = 12345;
  auto next = [&]() { seed = seed * 1664525u + 1013904223u; return int16_t(int(seed >> 16) % 20000 - 10000); };
  {
    std::vector<cs> x[2] = {std::vector<cs>(64 * 32 * 2 + 5), std::vector<cs>(12 * 300 + 1)};
    for (int i = 0; i < 2; i++) for (size_t k = 0; k < x[i].size(); k++) x[i][k] = cs(next(), next());
    const int selv[3] = {11, 0, 5};
    const std::vector<int> sel(selv, selv + 3);
    gpu::Channelizer<int16_t> a(64, 32, prototype(64, 64)), b(12, 6, prototype(12, 30), sel), ta(64, 32, prototype(64, 64)), tb(12, 6, prototype(12, 30), sel);
    gpu::Channelizer<int16_t> *nodes[4] = {&a, &b, &ta, &tb};
    failures += runPair<gpu::Channelizer<int16_t>, cs, cf>("Channelizer<int16_t>", nodes, x);
  }
  {
    std::vector<int16_t> x[2] = {std::vector<int16_t>(64 * 32 * 2 + 5), std::vector<int16_t>(12 * 300 + 1)};
    for (int i = 0; i < 2; i++) for (size_t k = 0; k < x[i].size(); k++) x[i][k] = next();
    const int selv[3] = {6, 0, 3}, modev[3] = {SDRHIP_EPI_FM, SDRHIP_EPI_AM, SDRHIP_EPI_USB};
    const float gainv[3] = {0.5f, 1.5f, 0.75f};
    const std::vector<int> sel(selv, selv + 3), modes(modev, modev + 3);
    const std::vector<float> gains(gainv, gainv + 3);
    typedef gpu::RealAudioChannelizer<int16_t> Node;
    Node a(64, 32, prototype(64, 64)), b(12, 6, prototype(12, 30), sel, modes, gains), ta(64, 32, prototype(64, 64)), tb(12, 6, prototype(12, 30), sel, modes, gains);
    Node *nodes[4] = {&a, &b, &ta, &tb};
    failures += runPair<Node, int16_t, int16_t>("RealAudioChannelizer<int16_t>", nodes, x);
  }
  return failures;
}

int main(int argc, char **argv) {
  return runMain("usage: test_changroup rules | gpu\n", [&]() -> int {
    if (argc >= 2 && std::string(argv[1]) == "rules") return runRules();
    if (argc >= 2 && std::string(argv[1]) == "gpu") return runGpu();
    return -1;
  });
}
