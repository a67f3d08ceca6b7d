// cut.cc — cuts the g23_baudot_* fixtures of the Baudot decoder bank from the UNMODIFIED reference node (sdr::Baudot) and times
// the node on one core. TEST INFRASTRUCTURE: our own driver; it only includes the reference's headers at build time and links
// its objects where they lie (tools/golden_baudot/Makefile builds outside the tree).
//
//   cut golden <dir>     reads <dir>/g23_baudot_inputs.txt and g23_baudot_bits.bin (make_inputs.py), writes
//                        <dir>/manifest_baudot.json: per case the splits, after every call the node's state
//                        [_bitstream, _bitcount, _mode] and what the call sent (hex text, or null where it sent nothing)
//   cut bench <rows.bin> <rows> <bits> <stop>   ms per call of `rows` nodes over one row each, JSON on stdout
//
// The reference sizes its output buffer bufferSize / (2 * bitsPerSymbol) + 1 and indexes it unchecked, while a call of n
// half-bits can complete ceil(n / bitsPerSymbol) symbols. The node never compares a call's length with the declared size, so
// the feeder declares a bufferSize of 2 n + 32 for calls of at most n half-bits: the unmodified node stays inside its buffer.
#include "node.hh"
#include "baudot.hh"

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
  void configure(size_t maxlen) { this->setConfig(Config(Config::typeId<uint8_t>(), 90.90, 2 * maxlen + 32, 1)); }
  void feed(uint8_t *p, size_t n) { Buffer<uint8_t> view(p, n); this->send(view, false); }
};

class Probe : public Baudot {
public:
  explicit Probe(StopBits s) : Baudot(s) {}
  std::string state() const {
    char buf[96];
    snprintf(buf, sizeof buf, "[%u, %llu, %d]", unsigned(_bitstream), (unsigned long long)_bitcount, int(_mode));
    return buf;
  }
};

class Collector : public Sink<uint8_t> {
public:
  Collector() : sent(false), chars(0) {}
  bool sent;
  std::string hex;
  size_t chars;
  virtual void config(const Config &) {}
  virtual void process(const Buffer<uint8_t> &buffer, bool) {
    sent = true;
    char h[4];
    for (size_t i = 0; i < buffer.size(); i++) { snprintf(h, sizeof h, "%02x", unsigned(buffer[i])); hex += h; }
    chars += buffer.size();
  }
};

static std::vector<uint8_t> slurp(const std::string &path) {
  std::ifstream f(path.c_str(), std::ios::binary);
  if (!f) { perror(path.c_str()); exit(2); }
  return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

static int golden(const std::string &dir) {
  std::vector<uint8_t> bits = slurp(dir + "/g23_baudot_bits.bin");
  std::ifstream idx((dir + "/g23_baudot_inputs.txt").c_str());
  if (!idx) { perror("g23_baudot_inputs.txt"); return 2; }
  std::ostringstream js;
  js << "{\n \"bits\": {\"file\": \"g23_baudot_bits.bin\", \"dtype\": \"u8\", \"count\": " << bits.size() << "},\n \"cases\": [\n";
  std::string name;
  int stop;
  size_t offset, n, ns, total = 0;
  bool first = true;
  while (idx >> name >> stop >> offset >> n >> ns) {
    std::vector<size_t> splits(ns);
    size_t longest = 1;
    for (size_t i = 0; i < ns; i++) { idx >> splits[i]; longest = std::max(longest, splits[i]); }
    if (offset + n > bits.size()) { fprintf(stderr, "%s: row behind the bits\n", name.c_str()); return 2; }
    Feeder src;
    Probe node(stop == 0 ? Baudot::STOP1 : stop == 1 ? Baudot::STOP15 : Baudot::STOP2);
    Collector sink;
    src.connect(&node, true);
    node.connect(&sink, true);
    src.configure(longest);
    js << (first ? "" : ",\n") << "  {\"name\": \"" << name << "\", \"stop\": " << stop << ", \"offset\": " << offset << ", \"n\": " << n << ", \"splits\": [";
    first = false;
    std::ostringstream states, sends;
    size_t at = offset;
    for (size_t i = 0; i < ns; i++) {
      sink.sent = false;
      sink.hex.clear();
      src.feed(bits.data() + at, splits[i]);
      at += splits[i];
      js << (i ? ", " : "") << splits[i];
      states << (i ? ", " : "") << node.state();
      if (sink.sent) sends << (i ? ", " : "") << "\"" << sink.hex << "\"";
      else sends << (i ? ", " : "") << "null";
    }
    js << "],\n   \"states\": [" << states.str() << "],\n   \"sends\": [" << sends.str() << "]}";
    total += sink.chars;
  }
  js << "\n ],\n \"characters\": " << total << "\n}\n";
  FILE *f = fopen((dir + "/manifest_baudot.json").c_str(), "w");
  if (!f) { perror("manifest_baudot.json"); return 2; }
  fputs(js.str().c_str(), f);
  fclose(f);
  return 0;
}

// `rows` nodes, one row of `n` half-bits each — what the decoder bank does in one call — on one core; the median of `reps` passes
static int bench(const std::string &path, size_t rows, size_t n, int stop, int reps) {
  std::vector<uint8_t> bits = slurp(path);
  if (bits.size() < rows * n) { fprintf(stderr, "%s: %zu bytes < %zu\n", path.c_str(), bits.size(), rows * n); return 2; }
  const Baudot::StopBits sb = stop == 0 ? Baudot::STOP1 : stop == 1 ? Baudot::STOP15 : Baudot::STOP2;
  std::vector<double> ms;
  size_t chars = 0;
  for (int r = -1; r < reps; r++) {
    std::vector<Feeder> src(rows);
    std::vector<Probe *> node(rows);
    std::vector<Collector> sink(rows);
    for (size_t c = 0; c < rows; c++) {
      node[c] = new Probe(sb);
      src[c].connect(node[c], true);
      node[c]->connect(&sink[c], true);
      src[c].configure(n);
    }
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    for (size_t c = 0; c < rows; c++) src[c].feed(bits.data() + c * n, n);
    const double dt = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (r >= 0) ms.push_back(dt);
    chars = 0;
    for (size_t c = 0; c < rows; c++) { chars += sink[c].chars; delete node[c]; }
  }
  std::sort(ms.begin(), ms.end());
  printf("{\"rows\": %zu, \"n\": %zu, \"reps\": %d, \"characters\": %zu, \"cpu_reference_ms\": %.4f, \"min_ms\": %.4f, \"max_ms\": %.4f}\n", rows, n,
         reps, chars, ms[ms.size() / 2], ms.front(), ms.back());
  return 0;
}

int main(int argc, char **argv) {
  if (argc >= 3 && std::string(argv[1]) == "golden") return golden(argv[2]);
  if (argc >= 6 && std::string(argv[1]) == "bench")
    return bench(argv[2], strtoul(argv[3], 0, 10), strtoul(argv[4], 0, 10), atoi(argv[5]), 9);
  fprintf(stderr, "usage: cut golden <dir> | cut bench <rows.bin> <rows> <bits> <stop>\n");
  return 1;
}
