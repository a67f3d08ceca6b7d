// test_baudot.cc — sdr::gpu::Baudot and sdr::gpu::BaudotBank (include/sdr/gpu/baudot.hh) against the g23 fixtures cut from the
// reference (tests/golden/manifest_baudot.json, flattened by tests/test_cpp_baudot.py into cases.txt).
//   test_baudot --host-only                config() rules, no device needed
//   test_baudot <cases.txt> <bits.bin>     + Feeder -> gpu::Baudot -> TextSink delivers the fixtures' sends, call by call, and
//                                          every fixture row as one channel of ONE bank through process() and processDev()
// cases.txt, per case: name stop offset n calls, then per call: the split and what the call sent (hex, or - for no send).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "sdr/sdr.hh"
#include "sdr/gpu/baudot.hh"

using namespace sdr;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

struct Feeder : public Source {
  void cfg(Config::Type t, size_t bs) { setConfig(Config(t, 90.90, bs, 1)); }
  void feed(uint8_t *p, size_t n) { Buffer<uint8_t> b(p, n); send(b, false); }
};
struct TextSink : public Sink<uint8_t> {
  Config last;
  bool sent = false;
  std::string text;
  virtual void config(const Config &c) { last = c; }
  virtual void process(const Buffer<uint8_t> &b, bool) { sent = true; text.assign(reinterpret_cast<const char *>(b.data()), b.size()); }
};

// gpu::Baudot with its three device calls recorded in place of made: what config() decides needs no device
struct Planned : public gpu::Baudot {
  explicit Planned(StopBits s) : gpu::Baudot(s), now(LETTERS) {}
  std::vector<std::string> log;
  Mode now;
  virtual void createPlan(size_t maxBits, Mode mode) { log.push_back("create " + std::to_string(maxBits) + (mode == FIGURES ? " FIGURES" : " LETTERS")); now = mode; }
  virtual void resetPlan() { log.push_back("reset keep_mode"); }
  virtual Mode planMode() { return now; }
};

static void testHostOnly() {
  gpu::Baudot node;   // the reference's default: STOP15
  node.config(Config());   // nothing known yet: silent
  bool threw = false;
  try { node.config(Config(Config::Type_s16, 90.90, 512, 1)); } catch (ConfigError &e) {
    threw = std::string(e.what()).find("Can not configure Baudot: Invalid type") != std::string::npos;
  }
  CHECK(threw);
  try { node.config(Config(Config::Type_u8, 90.90, 512, 1)); } catch (ConfigError &) {}   // without a device: a ConfigError, never a crash
  CHECK(int(gpu::Baudot::STOP1) == SDRHIP_BAUDOT_STOP1 && int(gpu::Baudot::STOP15) == SDRHIP_BAUDOT_STOP15 && int(gpu::Baudot::STOP2) == SDRHIP_BAUDOT_STOP2);
  CHECK(int(gpu::Baudot::LETTERS) == SDRHIP_BAUDOT_LETTERS && int(gpu::Baudot::FIGURES) == SDRHIP_BAUDOT_FIGURES);

  // the re-config() rule: a first config() makes a fresh node, a later one is config() on the old node — the registers start
  // over, the table stays — and a larger buffer makes a new node that starts in the old one's table
  Planned p(gpu::Baudot::STOP1);
  TextSink out;
  p.connect(&out, true);
  CHECK(p.mode() == gpu::Baudot::LETTERS);
  p.config(Config(Config::Type_u8, 90.90, 446, 1));
  CHECK(p.log.size() == 1 && p.log[0] == "create 446 LETTERS");
  CHECK(out.last.type() == Config::Type_u8 && out.last.bufferSize() == 446 / 14 + 1);   // the capacity, not the reference's half of it
  p.now = gpu::Baudot::FIGURES;   // (the node has met a figures shift)
  p.config(Config(Config::Type_u8, 90.90, 446, 1));
  CHECK(p.log.size() == 2 && p.log[1] == "reset keep_mode" && p.mode() == gpu::Baudot::FIGURES);
  p.config(Config(Config::Type_u8, 90.90, 100, 1));
  CHECK(p.log.size() == 3 && p.log[2] == "reset keep_mode" && out.last.bufferSize() == 100 / 14 + 1);
  p.config(Config(Config::Type_u8, 90.90, 1000, 1));
  CHECK(p.log.size() == 4 && p.log[3] == "create 1000 FIGURES" && out.last.bufferSize() == 1000 / 14 + 1);
  threw = false;
  try { p.config(Config(Config::Type_cs16, 90.90, 1000, 1)); } catch (ConfigError &) { threw = true; }
  CHECK(threw && p.log.size() == 4);
}

struct Call { size_t n; bool sent; std::string text; };
struct Case { std::string name; int stop; size_t offset, n; std::vector<Call> calls; };

static std::string unhex(const std::string &h) {
  std::string out;
  for (size_t i = 0; i + 1 < h.size(); i += 2) out.push_back(char(std::stoi(h.substr(i, 2), 0, 16)));
  return out;
}

static std::vector<Case> load(const char *path) {
  std::ifstream f(path);
  std::vector<Case> out;
  Case c;
  size_t calls;
  while (f >> c.name >> c.stop >> c.offset >> c.n >> calls) {
    c.calls.resize(calls);
    for (size_t k = 0; k < calls; k++) {
      std::string send;
      f >> c.calls[k].n >> send;
      c.calls[k].sent = send != "-";
      c.calls[k].text = c.calls[k].sent ? unhex(send) : std::string();
    }
    out.push_back(c);
  }
  return out;
}

static gpu::Baudot::StopBits stopOf(int s) { return s == 0 ? gpu::Baudot::STOP1 : s == 1 ? gpu::Baudot::STOP15 : gpu::Baudot::STOP2; }

// the reference's graph: source -> Baudot -> sink; a call that decodes nothing sends nothing
static void testGraph(const std::vector<Case> &cases, std::vector<uint8_t> &bits) {
  size_t sends = 0;
  for (size_t i = 0; i < cases.size(); i++) {
    const Case &c = cases[i];
    Feeder src;
    gpu::Baudot node(stopOf(c.stop));
    TextSink out;
    src.connect(&node, true);
    node.connect(&out, true);
    size_t longest = 1;
    for (size_t k = 0; k < c.calls.size(); k++) longest = std::max(longest, c.calls[k].n);
    src.cfg(Config::Type_u8, longest);
    CHECK(out.last.type() == Config::Type_u8 && out.last.bufferSize() == longest / 14 + 1);
    size_t at = c.offset;
    for (size_t k = 0; k < c.calls.size(); k++) {
      out.sent = false;
      out.text.clear();
      src.feed(bits.data() + at, c.calls[k].n);
      at += c.calls[k].n;
      if (out.sent != c.calls[k].sent || out.text != c.calls[k].text) {
        std::printf("FAIL graph %s: call %zu sent %d '%s', want %d '%s'\n", c.name.c_str(), k, int(out.sent), out.text.c_str(), int(c.calls[k].sent),
                    c.calls[k].text.c_str());
        failures++;
        break;
      }
      sends += out.sent;
    }
    if (i == 1) {   // config() again in mid-stream: the registers start over, the table stays, and the node decodes on
      const gpu::Baudot::Mode m = node.mode();
      src.cfg(Config::Type_u8, longest);
      CHECK(node.mode() == m);
    }
  }
  CHECK(sends > 100);
  std::printf("graph: %zu cases, %zu sends\n", cases.size(), sends);
}

static void compareBank(const char *what, const gpu::BaudotBank &bank, const std::vector<Case> &cases, size_t k, size_t &chars) {
  for (size_t c = 0; c < cases.size(); c++) {
    const std::string want = k < cases[c].calls.size() ? cases[c].calls[k].text : std::string();
    if (bank.text(c) != want) {
      std::printf("FAIL %s %s: call %zu '%s', want '%s'\n", what, cases[c].name.c_str(), k, bank.text(c).c_str(), want.c_str());
      failures++;
    }
    chars += want.size();
  }
}

static void testBank(const std::vector<Case> &cases, const std::vector<uint8_t> &bits) {
  const size_t C = cases.size();
  size_t calls = 0, maxBits = 1;
  std::vector<gpu::Baudot::StopBits> stops(C);
  for (size_t c = 0; c < C; c++) {
    calls = std::max(calls, cases[c].calls.size());
    stops[c] = stopOf(cases[c].stop);
    for (size_t k = 0; k < cases[c].calls.size(); k++) maxBits = std::max(maxBits, cases[c].calls[k].n);
  }
  const size_t stride = maxBits + 7;
  gpu::BaudotBank host(stops, maxBits), dev(stops, maxBits);
  sdrhip_ctx *ctx = gpu::Device::get(0);
  gpu::detail::DeviceMem dbits, dcounts;
  dbits.alloc(ctx, C * stride, "test");
  dcounts.alloc(ctx, C * sizeof(uint32_t), "test");
  std::vector<uint8_t> buf(C * stride);
  std::vector<uint32_t> counts(C);
  std::vector<size_t> at(C);
  for (size_t c = 0; c < C; c++) at[c] = cases[c].offset;
  size_t chars = 0;
  for (size_t k = 0; k < calls; k++) {
    std::fill(buf.begin(), buf.end(), uint8_t(0xA5));   // bit 0 set behind every count
    for (size_t c = 0; c < C; c++) {
      counts[c] = k < cases[c].calls.size() ? uint32_t(cases[c].calls[k].n) : 0;
      std::copy(bits.begin() + at[c], bits.begin() + at[c] + counts[c], buf.begin() + c * stride);
      at[c] += counts[c];
    }
    if (!host.process(buf.data(), stride, counts.data())) { std::printf("FAIL: process, call %zu\n", k); failures++; }
    gpu::detail::configCheck(sdrhip_memcpy_h2d_async(ctx, dbits.get(), buf.data(), buf.size()), "test");
    gpu::detail::configCheck(sdrhip_memcpy_h2d_async(ctx, dcounts.get(), counts.data(), C * sizeof(uint32_t)), "test");
    if (!dev.processDev(dbits.as<uint8_t>(), stride, dcounts.as<uint32_t>())) { std::printf("FAIL: processDev, call %zu\n", k); failures++; }
    compareBank("process", host, cases, k, chars);
    compareBank("processDev", dev, cases, k, chars);
    if (failures > 20) break;
  }
  CHECK(chars > 1000);
  std::printf("process, processDev: %zu channels, %zu calls, %zu characters\n", C, calls, chars);
  // a reset bank is a fresh one; a row switched off yields nothing; setChannel gives a row another setting
  host.reset();
  host.setEnabled(1, false);
  std::fill(counts.begin(), counts.end(), 0u);
  std::fill(buf.begin(), buf.end(), uint8_t(0xA5));
  size_t first = C, other = C;   // two one-call cases of different settings
  for (size_t c = 0; c < C; c++) {
    if (cases[c].calls.size() != 1 || cases[c].calls[0].text.empty()) continue;
    if (first == C) first = c;
    else if (other == C && cases[c].stop != cases[first].stop && cases[c].name.compare(0, 4, "text") == 0) other = c;
  }
  CHECK(first < C && other < C);
  if (first < C && other < C) {
    for (size_t c = 0; c < 3; c++) {   // rows 0 and 1: the first case; row 2: the other one, in that case's setting
      const Case &s = cases[c < 2 ? first : other];
      counts[c] = uint32_t(s.n);
      std::copy(bits.begin() + s.offset, bits.begin() + s.offset + s.n, buf.begin() + c * stride);
    }
    host.setChannel(0, stopOf(cases[first].stop));
    host.setChannel(1, stopOf(cases[first].stop));
    host.setChannel(2, stopOf(cases[other].stop));
    CHECK(host.process(buf.data(), stride, counts.data()));
    CHECK(host.text(0) == cases[first].calls[0].text && host.text(1).empty() && host.text(2) == cases[other].calls[0].text);
  }
}

int main(int argc, char **argv) {
  try {
    testHostOnly();
    if (argc >= 3) {
      const std::vector<Case> cases = load(argv[1]);
      std::ifstream fb(argv[2], std::ios::binary);
      std::vector<uint8_t> bits((std::istreambuf_iterator<char>(fb)), std::istreambuf_iterator<char>());
      CHECK(cases.size() >= 54 && !bits.empty());
      testGraph(cases, bits);
      testBank(cases, bits);
    }
  } catch (std::exception &e) { std::printf("FAIL: exception: %s\n", e.what()); return 2; }
  std::printf("%s (%d failures)\n", failures ? "FAILED" : "OK", failures);
  return failures ? 1 : 0;
}
