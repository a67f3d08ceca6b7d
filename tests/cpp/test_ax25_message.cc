// test_ax25_message.cc — sdr::gpu::ax25::Address and Message (include/sdr/gpu/ax25_message.hh) on the CPU, no HIP: every frame the
// reference delivered in the g24 fixtures (tests/golden/manifest_ax25.json, flattened by tests/test_cpp_ax25_message.py) parses
// into the reference's to / from / via / payload and prints as the reference's AX25Dump printed it; frames shorter than their
// address field are malformed, and nothing behind a frame is read — every frame lies in a heap block of exactly its size.
//   test_ax25_message <frames.txt>
// frames.txt, per frame: raw to_call to_ssid from_call from_ssid n_via {call ssid} payload text — bytes in hex, - for none.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "sdr/gpu/ax25_message.hh"

using namespace sdr::gpu::ax25;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

static std::string unhex(const std::string &h) {
  std::string out;
  if (h == "-") return out;
  for (size_t i = 0; i + 1 < h.size(); i += 2) out.push_back(char(std::stoi(h.substr(i, 2), 0, 16)));
  return out;
}

// the frame in a heap block of exactly its size: a read behind it is the sanitizer's to find
static Message parse(const std::string &raw) {
  uint8_t *p = new uint8_t[raw.size()];
  if (!raw.empty()) memcpy(p, raw.data(), raw.size());
  Message m(p, raw.size());
  delete[] p;
  return m;
}

static std::string field(const std::string &call, unsigned ssid, bool last) {
  std::string f(7, char(' ' << 1));
  for (size_t i = 0; i < call.size() && i < 6; i++) f[i] = char(call[i] << 1);
  f[6] = char(0x60 | (ssid << 1) | (last ? 1 : 0));
  return f;
}

static void testFixtures(const char *path) {
  std::ifstream f(path);
  std::string raw, toCall, fromCall, payload, text;
  size_t toSsid, fromSsid, nVia, frames = 0;
  while (f >> raw >> toCall >> toSsid >> fromCall >> fromSsid >> nVia) {
    std::vector<std::pair<std::string, size_t> > via(nVia);
    for (size_t i = 0; i < nVia; i++) f >> via[i].first >> via[i].second;
    f >> payload >> text;
    const Message m = parse(unhex(raw));
    bool ok = !m.malformed() && m.to().call() == unhex(toCall) && m.to().ssid() == toSsid && m.from().call() == unhex(fromCall) &&
              m.from().ssid() == fromSsid && m.via().size() == nVia && m.payload() == unhex(payload) && m.raw() == unhex(raw);
    for (size_t i = 0; ok && i < nVia; i++) ok = m.via()[i].call() == unhex(via[i].first) && m.via()[i].ssid() == via[i].second;
    std::ostringstream dump;
    dump << "AX25: " << m << std::endl;   // AX25Dump::handleAX25Message
    ok = ok && dump.str() == "AX25: " + unhex(text) + "\n";
    if (!ok) { std::printf("FAIL frame %zu: %s\n", frames, dump.str().c_str()); failures++; }
    frames++;
  }
  std::printf("%zu frames\n", frames);
}

static void testMalformed() {
  const std::string good = field("APRS", 0, false) + field("DL1ABC", 9, false) + field("WIDE1", 1, true) + "\x03\xf0hi";
  const Message m = parse(good);
  std::ostringstream s;
  s << m;
  CHECK(!m.malformed() && s.str() == "DL1ABC-9 > APRS-0 via WIDE1-1 N=4\n\x03\xf0hi");
  CHECK(m.to().call() == "APRS" && !m.to().isEmpty() && m.from().ssid() == 9 && m.via().size() == 1 && m.payload().size() == 4);
  const Message two = parse(good.substr(0, 7) + field("K1XYZ", 2, true));
  CHECK(!two.malformed() && two.via().empty() && two.payload().empty() && two.from().call() == "K1XYZ");
  std::string endless = field("A", 0, false) + field("B", 0, false);
  for (int i = 0; i < 3; i++) endless += field("C", 0, false);   // no address says it is the last
  const std::string bad[] = {std::string(), good.substr(0, 6), good.substr(0, 13), good.substr(0, 14), good.substr(0, 20), endless};
  for (size_t i = 0; i < sizeof bad / sizeof bad[0]; i++) {
    const Message b = parse(bad[i]);
    std::ostringstream t;
    t << b;
    CHECK(b.malformed() && b.raw() == bad[i] && b.via().empty() && b.to().isEmpty() && b.from().isEmpty() && b.payload().empty());
    CHECK(t.str() == "malformed N=" + std::to_string(bad[i].size()) + "\n" + bad[i]);
  }
  bool ext = false;
  CHECK(Address::unpack(reinterpret_cast<const uint8_t *>(field("AB CD", 3, false).data()), ext).call() == "AB C" && ext);   // cut as the reference cuts
  CHECK(Message().via().empty() && !Message().malformed() && Address().isEmpty() && Address("X", 5).ssid() == 5);
}

int main(int argc, char **argv) {
  testMalformed();
  if (argc >= 2) testFixtures(argv[1]);
  std::printf("%s (%d failures)\n", failures ? "FAILED" : "OK", failures);
  return failures ? 1 : 0;
}
