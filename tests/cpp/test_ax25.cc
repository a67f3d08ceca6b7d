// test_ax25.cc — sdr::gpu::AX25, AX25Dump and AX25Bank (include/sdr/gpu/ax25.hh) against the g24 fixtures cut from the reference
// (tests/golden/manifest_ax25.json, flattened by tests/test_cpp_ax25.py into cases.txt).
//   test_ax25 --host-only                config() rules, no device needed
//   test_ax25 <cases.txt> <bits.bin>     + Feeder -> gpu::AX25 delivers the fixtures' messages, call by call, and every fixture
//                                        row as one channel of ONE bank through process() and processDev()
// cases.txt, per case: name offset n calls, then per call: the split, the number of frames and per frame raw and text (hex).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <sstream>
#include <string>
#include <vector>

#include "sdr/sdr.hh"
#include "sdr/gpu/ax25.hh"

using namespace sdr;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

struct Feeder : public Source {
  void cfg(Config::Type t, size_t bs) { setConfig(Config(t, 1200, bs, 1)); }
  void feed(uint8_t *p, size_t n) { Buffer<uint8_t> b(p, n); send(b, false); }
};

// the messages of one call: their raw bytes and their text
struct MessageLog : public gpu::AX25 {
  std::vector<std::string> raw, text;
  virtual void handleAX25Message(const Message &m) {
    std::ostringstream s;
    s << m;
    raw.push_back(m.raw());
    text.push_back(s.str());
  }
};

// gpu::AX25 with its two device calls recorded in place of made: what config() decides needs no device
struct Planned : public gpu::AX25 {
  std::vector<std::string> log;
  virtual void createPlan(size_t maxBits) { log.push_back("create " + std::to_string(maxBits)); }
  virtual void resetPlan() { log.push_back("reset"); }
};

static void testHostOnly() {
  gpu::AX25 node;
  node.config(Config());   // nothing known yet: silent
  bool threw = false;
  try { node.config(Config(Config::Type_s16, 1200, 512, 1)); } catch (ConfigError &e) {
    threw = std::string(e.what()).find("Can not configure AX25: Invalid type") != std::string::npos;
  }
  CHECK(threw);
  try { node.config(Config(Config::Type_u8, 1200, 512, 1)); } catch (ConfigError &) {}   // without a device: a ConfigError, never a crash
  // every config() is a node that starts over: a first one makes the device node, a later one resets it, a larger buffer makes
  // a new one
  Planned p;
  p.config(Config(Config::Type_u8, 1200, 446, 1));
  p.config(Config(Config::Type_u8, 1200, 446, 1));
  p.config(Config(Config::Type_u8, 1200, 100, 1));
  p.config(Config(Config::Type_u8, 1200, 1000, 1));
  CHECK(p.log.size() == 4 && p.log[0] == "create 446" && p.log[1] == "reset" && p.log[2] == "reset" && p.log[3] == "create 1000");
  threw = false;
  try { p.config(Config(Config::Type_cs16, 1200, 1000, 1)); } catch (ConfigError &) { threw = true; }
  CHECK(threw && p.log.size() == 4);
  // the dump's text, through the node's own virtual call
  std::ostringstream out;
  gpu::AX25Dump dump(out);
  const uint8_t f[] = {'A' << 1, 'P' << 1, 'R' << 1, 'S' << 1, ' ' << 1, ' ' << 1, 0x60, 'N' << 1, '0' << 1, 'C' << 1, 'A' << 1, 'L' << 1, 'L' << 1, 0x6f, 0x03, 0xf0, '>'};
  dump.handleAX25Message(gpu::AX25::Message(f, sizeof f));
  CHECK(out.str() == "AX25: N0CALL-7 > APRS-0 N=3\n\x03\xf0>\n");
}

struct Call { size_t n; std::vector<std::string> raw, text; };
struct Case { std::string name; size_t offset, n; std::vector<Call> calls; };

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
  while (f >> c.name >> c.offset >> c.n >> calls) {
    c.calls.assign(calls, Call());
    for (size_t k = 0; k < calls; k++) {
      size_t frames;
      f >> c.calls[k].n >> frames;
      for (size_t i = 0; i < frames; i++) {
        std::string raw, text;
        f >> raw >> text;
        c.calls[k].raw.push_back(unhex(raw));
        c.calls[k].text.push_back(unhex(text));
      }
    }
    out.push_back(c);
  }
  return out;
}

// the reference's graph: source -> AX25, which hands its frames to the virtual call
static void testGraph(const std::vector<Case> &cases, std::vector<uint8_t> &bits) {
  size_t messages = 0;
  for (size_t i = 0; i < cases.size(); i++) {
    const Case &c = cases[i];
    Feeder src;
    MessageLog node;
    src.connect(&node, true);
    size_t longest = 1;
    for (size_t k = 0; k < c.calls.size(); k++) longest = std::max(longest, c.calls[k].n);
    src.cfg(Config::Type_u8, longest);
    size_t at = c.offset;
    for (size_t k = 0; k < c.calls.size(); k++) {
      node.raw.clear();
      node.text.clear();
      src.feed(bits.data() + at, c.calls[k].n);
      at += c.calls[k].n;
      if (node.raw != c.calls[k].raw || node.text != c.calls[k].text) {
        std::printf("FAIL graph %s: call %zu delivered %zu messages, want %zu\n", c.name.c_str(), k, node.raw.size(), c.calls[k].raw.size());
        failures++;
        break;
      }
      messages += node.raw.size();
    }
  }
  CHECK(messages >= 30);
  std::printf("graph: %zu cases, %zu messages\n", cases.size(), messages);
}

static void compareBank(const char *what, const gpu::AX25Bank &bank, const std::vector<Case> &cases, size_t k, size_t &messages) {
  for (size_t c = 0; c < cases.size(); c++) {
    static const Call none = Call();
    const Call &want = k < cases[c].calls.size() ? cases[c].calls[k] : none;
    bool ok = bank.frameCount(c) == want.raw.size();
    for (size_t i = 0; ok && i < want.raw.size(); i++) {
      std::ostringstream s;
      s << bank.message(c, i);
      ok = bank.message(c, i).raw() == want.raw[i] && s.str() == want.text[i] && bank.bitIndex(c, i) < want.n;
    }
    if (!ok) {
      std::printf("FAIL %s %s: call %zu, %zu frames, want %zu\n", what, cases[c].name.c_str(), k, bank.frameCount(c), want.raw.size());
      failures++;
    }
    messages += want.raw.size();
  }
}

static void testBank(const std::vector<Case> &cases, const std::vector<uint8_t> &bits) {
  const size_t C = cases.size();
  size_t calls = 0, maxBits = 1;
  for (size_t c = 0; c < C; c++) {
    calls = std::max(calls, cases[c].calls.size());
    for (size_t k = 0; k < cases[c].calls.size(); k++) maxBits = std::max(maxBits, cases[c].calls[k].n);
  }
  const size_t stride = maxBits + 7;
  gpu::AX25Bank host(C, maxBits), dev(C, maxBits);
  sdrhip_ctx *ctx = gpu::Device::get(0);
  gpu::detail::DeviceMem dbits, dcounts;
  dbits.alloc(ctx, C * stride, "test");
  dcounts.alloc(ctx, C * sizeof(uint32_t), "test");
  std::vector<uint8_t> buf(C * stride);
  std::vector<uint32_t> counts(C);
  std::vector<size_t> at(C);
  for (size_t c = 0; c < C; c++) at[c] = cases[c].offset;
  size_t messages = 0;
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
    compareBank("process", host, cases, k, messages);
    compareBank("processDev", dev, cases, k, messages);
    if (failures > 20) break;
  }
  CHECK(messages >= 60);
  std::printf("process, processDev: %zu channels, %zu calls, %zu messages\n", C, calls, messages);
  // a reset bank is a fresh one, and a row switched off yields nothing: a one-call case on rows 0 and 1
  host.reset();
  host.setEnabled(1, false);
  size_t one = C;
  for (size_t c = 0; c < C && one == C; c++)
    if (cases[c].calls.size() == 1 && !cases[c].calls[0].raw.empty()) one = c;
  CHECK(one < C);
  if (one < C) {
    std::fill(counts.begin(), counts.end(), 0u);
    for (size_t c = 0; c < 2; c++) {
      counts[c] = uint32_t(cases[one].n);
      std::copy(bits.begin() + cases[one].offset, bits.begin() + cases[one].offset + cases[one].n, buf.begin() + c * stride);
    }
    CHECK(host.process(buf.data(), stride, counts.data()));
    CHECK(host.frameCount(0) == cases[one].calls[0].raw.size() && host.frameCount(1) == 0 && host.message(0, 0).raw() == cases[one].calls[0].raw[0]);
    host.resetChannel(0);
    host.setEnabled(1, true);
    CHECK(host.process(buf.data(), stride, counts.data()));
    CHECK(host.frameCount(0) == host.frameCount(1) && host.frameCount(1) == cases[one].calls[0].raw.size());
  }
}

int main(int argc, char **argv) {
  try {
    testHostOnly();
    if (argc >= 3) {
      const std::vector<Case> cases = load(argv[1]);
      std::ifstream fb(argv[2], std::ios::binary);
      std::vector<uint8_t> bits((std::istreambuf_iterator<char>(fb)), std::istreambuf_iterator<char>());
      CHECK(cases.size() >= 16 && !bits.empty());
      testGraph(cases, bits);
      testBank(cases, bits);
    }
  } catch (std::exception &e) { std::printf("FAIL: exception: %s\n", e.what()); return 2; }
  std::printf("%s (%d failures)\n", failures ? "FAILED" : "OK", failures);
  return failures ? 1 : 0;
}
