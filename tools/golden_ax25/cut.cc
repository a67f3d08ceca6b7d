// cut.cc — cuts the g24_ax25_* fixtures of the AX.25 deframer bank from the UNMODIFIED reference node (sdr::AX25) and times the
// node on one core. TEST INFRASTRUCTURE: our own driver; it only includes the reference's headers at build time and links its
// objects where they lie (tools/golden_ax25/Makefile builds outside the tree).
//
//   cut golden <dir>     reads <dir>/g24_ax25_inputs.txt and g24_ax25_bits.bin (make_inputs.py), writes <dir>/manifest_ax25.json:
//                        per case the splits; after every call the node's protected state [_bitstream, _bitbuffer, _state, len,
//                        FNV-1a of _rxbuffer[0:len]]; after the last call _rxbuffer[0:len] itself; and per call the frames
//                        handleAX25Message saw: the raw bytes read from _rxbuffer, to / from / via as [call, ssid], the payload and
//                        the text of the reference's operator<< — all bytes in hex
//   cut bench <rows.bin> <rows> <bits>   ms per call of `rows` nodes over one row each, JSON on stdout
//
// The reference's Message constructor reads behind a frame that is shorter than its address field; the input rows hold no such
// frame that passes the CRC.
#include "node.hh"
#include "ax25.hh"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <sstream>
#include <string>
#include <vector>

using namespace sdr;

class Feeder : public Source {
public:
  void configure(size_t maxlen) { this->setConfig(Config(Config::typeId<uint8_t>(), 1200, maxlen + 1, 1)); }
  void feed(uint8_t *p, size_t n) { Buffer<uint8_t> view(p, n); this->send(view, false); }
};

static std::string hex(const uint8_t *p, size_t n) {
  std::string s;
  char h[4];
  for (size_t i = 0; i < n; i++) { snprintf(h, sizeof h, "%02x", unsigned(p[i])); s += h; }
  return s;
}
static std::string hex(const std::string &s) { return hex(reinterpret_cast<const uint8_t *>(s.data()), s.size()); }

static std::string address(const AX25::Address &a) {
  std::ostringstream o;
  o << "[\"" << hex(a.call()) << "\", " << a.ssid() << "]";
  return o.str();
}

class Probe : public AX25 {
public:
  Probe() : frames(0) {}
  size_t frames;
  std::string seen;   // the JSON of this call's frames
  virtual void handleAX25Message(const Message &msg) {
    std::ostringstream o, text;
    text << msg;
    o << (seen.empty() ? "" : ", ") << "{\"raw\": \"" << hex(_rxbuffer, size_t(_ptr - _rxbuffer) - 2) << "\", \"to\": " << address(msg.to())
      << ", \"from\": " << address(msg.from()) << ", \"via\": [";
    for (size_t i = 0; i < msg.via().size(); i++) o << (i ? ", " : "") << address(msg.via()[i]);
    o << "], \"payload\": \"" << hex(msg.payload()) << "\", \"text\": \"" << hex(text.str()) << "\"}";
    seen += o.str();
    frames++;
  }
  size_t len() const { return size_t(_ptr - _rxbuffer); }
  std::string state() const {
    unsigned fnv = 2166136261u;
    for (size_t i = 0; i < len(); i++) fnv = (fnv ^ _rxbuffer[i]) * 16777619u;
    char buf[128];
    snprintf(buf, sizeof buf, "[%u, %u, %u, %zu, %u]", unsigned(_bitstream), unsigned(_bitbuffer), unsigned(_state), len(), fnv);
    return buf;
  }
  std::string buffered() const { return hex(_rxbuffer, len()); }
};

static std::vector<uint8_t> slurp(const std::string &path) {
  std::ifstream f(path.c_str(), std::ios::binary);
  if (!f) { perror(path.c_str()); exit(2); }
  return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

static int golden(const std::string &dir) {
  std::vector<uint8_t> bits = slurp(dir + "/g24_ax25_bits.bin");
  std::ifstream idx((dir + "/g24_ax25_inputs.txt").c_str());
  if (!idx) { perror("g24_ax25_inputs.txt"); return 2; }
  std::ostringstream js;
  js << "{\n \"bits\": {\"file\": \"g24_ax25_bits.bin\", \"dtype\": \"u8\", \"count\": " << bits.size() << "},\n \"cases\": [\n";
  std::string name;
  size_t offset, n, ns, total = 0;
  bool first = true;
  while (idx >> name >> offset >> n >> ns) {
    std::vector<size_t> splits(ns);
    size_t longest = 1;
    for (size_t i = 0; i < ns; i++) { idx >> splits[i]; longest = std::max(longest, splits[i]); }
    if (offset + n > bits.size()) { fprintf(stderr, "%s: row behind the bits\n", name.c_str()); return 2; }
    Feeder src;
    Probe node;
    src.connect(&node, true);
    src.configure(longest);
    js << (first ? "" : ",\n") << "  {\"name\": \"" << name << "\", \"offset\": " << offset << ", \"n\": " << n << ", \"splits\": [";
    first = false;
    std::ostringstream states, frames;
    size_t at = offset;
    for (size_t i = 0; i < ns; i++) {
      node.seen.clear();
      src.feed(bits.data() + at, splits[i]);
      at += splits[i];
      js << (i ? ", " : "") << splits[i];
      states << (i ? ", " : "") << node.state();
      frames << (i ? ", " : "") << "[" << node.seen << "]";
    }
    js << "],\n   \"states\": [" << states.str() << "],\n   \"rxbuffer\": \"" << node.buffered() << "\",\n   \"frames\": [" << frames.str() << "]}";
    total += node.frames;
  }
  js << "\n ],\n \"frames\": " << total << "\n}\n";
  FILE *f = fopen((dir + "/manifest_ax25.json").c_str(), "w");
  if (!f) { perror("manifest_ax25.json"); return 2; }
  fputs(js.str().c_str(), f);
  fclose(f);
  return 0;
}

// `rows` nodes, one row of `n` bits each — what the deframer bank does in one call — on one core; the median of `reps` passes
static int bench(const std::string &path, size_t rows, size_t n, int reps) {
  std::vector<uint8_t> bits = slurp(path);
  if (bits.size() < rows * n) { fprintf(stderr, "%s: %zu bytes < %zu\n", path.c_str(), bits.size(), rows * n); return 2; }
  std::vector<double> ms;
  size_t frames = 0;
  for (int r = -1; r < reps; r++) {
    std::vector<Feeder> src(rows);
    std::vector<Probe *> node(rows);
    for (size_t c = 0; c < rows; c++) {
      node[c] = new Probe;
      src[c].connect(node[c], true);
      src[c].configure(n);
    }
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    for (size_t c = 0; c < rows; c++) src[c].feed(bits.data() + c * n, n);
    const double dt = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (r >= 0) ms.push_back(dt);
    frames = 0;
    for (size_t c = 0; c < rows; c++) { frames += node[c]->frames; delete node[c]; }
  }
  std::sort(ms.begin(), ms.end());
  printf("{\"rows\": %zu, \"n\": %zu, \"reps\": %d, \"frames\": %zu, \"cpu_reference_ms\": %.4f, \"min_ms\": %.4f, \"max_ms\": %.4f}\n", rows, n, reps,
         frames, ms[ms.size() / 2], ms.front(), ms.back());
  return 0;
}

int main(int argc, char **argv) {
  if (argc >= 3 && std::string(argv[1]) == "golden") return golden(argv[2]);
  if (argc >= 5 && std::string(argv[1]) == "bench") return bench(argv[2], strtoul(argv[3], 0, 10), strtoul(argv[4], 0, 10), 9);
  fprintf(stderr, "usage: cut golden <dir> | cut bench <rows.bin> <rows> <bits>\n");
  return 1;
}
