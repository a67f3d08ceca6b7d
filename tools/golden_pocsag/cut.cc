// cut.cc — cuts the g19_pocsag_* fixtures of the POCSAG decoder bank from the UNMODIFIED reference node (sdr::POCSAG) and
// pocsag_repair, and times the node on one core. TEST INFRASTRUCTURE: our own driver; it only includes the reference's
// headers at build time and links its objects where they lie (tools/golden_pocsag/Makefile builds outside the tree).
//
//   cut golden <dir>          (a message is recorded as address, function, bits, payload, estimateText, estimateNumeric, asNumeric)
//                             reads <dir>/g19_pocsag_inputs.txt, g19_pocsag_bits.bin, g19_pocsag_repair_in.bin (make_inputs.py)
//                             writes <dir>/manifest_pocsag.json and g19_pocsag_repair_out.bin (rc, word pairs)
//   cut bench <rows.bin> <rows> <bits>   ms per call of `rows` nodes over one row each, JSON on stdout
//
// The probe derives from sdr::POCSAG to read its protected state after every call and its queue at every handleMessages. It
// starts _bitcount and _slot at 0: the reference leaves them unset until the first sync word.
#include "node.hh"
#include "pocsag.hh"
#include "bch31_21.hh"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

using namespace sdr;

class Feeder : public Source {
public:
  void configure(size_t maxlen) { this->setConfig(Config(Config::typeId<uint8_t>(), 1200.0, maxlen, 1)); }
  void feed(uint8_t *p, size_t n) { Buffer<uint8_t> view(p, n); this->send(view, false); }
};

class Probe : public POCSAG {
public:
  Probe() : POCSAG(), call(0) { _bitcount = 0; _slot = 0; }
  int call;
  std::ostringstream deliveries;
  bool first = true;
  size_t n_messages = 0;
  virtual void handleMessages() {
    deliveries << (first ? "" : ", ") << "[" << call << ", [";
    first = false;
    bool f2 = true;
    for (std::list<Message>::iterator it = _queue.begin(); it != _queue.end(); ++it) {
      // the payload bytes are what asHex prints, but unpadded there: read them through a subclass view instead
      struct View : public Message { View(const Message &m) : Message(m) {} const std::vector<uint8_t> &bytes() const { return _payload; } };
      View v(*it);
      deliveries << (f2 ? "" : ", ") << "[" << it->address() << ", " << int(it->function()) << ", " << it->bits() << ", \"";
      char hex[4];
      for (size_t i = 0; i < v.bytes().size(); i++) { snprintf(hex, sizeof hex, "%02x", v.bytes()[i]); deliveries << hex; }
      deliveries << "\", " << it->estimateText() << ", " << it->estimateNumeric() << ", \"" << it->asNumeric() << "\"]";
      f2 = false;
      n_messages++;
    }
    deliveries << "]]";
    _queue.clear();
  }
  std::string state() const {
    char buf[96];
    snprintf(buf, sizeof buf, "[%d, %d, %d, \"%016llx\"]", int(_state), int(_bitcount), int(_slot), (unsigned long long)_bits);
    return buf;
  }
};

static std::vector<uint8_t> slurp(const std::string &path) {
  std::ifstream f(path.c_str(), std::ios::binary);
  if (!f) { perror(path.c_str()); exit(2); }
  return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

static int golden(const std::string &dir) {
  std::vector<uint8_t> bits = slurp(dir + "/g19_pocsag_bits.bin");
  std::ifstream idx((dir + "/g19_pocsag_inputs.txt").c_str());
  if (!idx) { perror("g19_pocsag_inputs.txt"); return 2; }
  std::ostringstream js;
  js << "{\n \"bits\": {\"file\": \"g19_pocsag_bits.bin\", \"dtype\": \"u8\", \"count\": " << bits.size() << "},\n \"cases\": [\n";
  std::string name;
  size_t n, ns, offset = 0, total_msgs = 0;
  bool first = true;
  while (idx >> name >> n >> ns) {
    std::vector<size_t> splits(ns);
    for (size_t i = 0; i < ns; i++) idx >> splits[i];
    Feeder src;
    Probe node;
    src.connect(&node, true);
    src.configure(65536);
    js << (first ? "" : ",\n") << "  {\"name\": \"" << name << "\", \"offset\": " << offset << ", \"n\": " << n << ", \"splits\": [";
    first = false;
    std::ostringstream states;
    size_t at = offset;
    for (size_t i = 0; i < ns; i++) {
      node.call = (int)i;
      src.feed(bits.data() + at, splits[i]);
      at += splits[i];
      js << (i ? ", " : "") << splits[i];
      states << (i ? ", " : "") << node.state();
    }
    js << "],\n   \"states\": [" << states.str() << "],\n   \"deliveries\": [" << node.deliveries.str() << "]}";
    offset += n;
    total_msgs += node.n_messages;
  }
  if (offset != bits.size()) { fprintf(stderr, "inputs.txt covers %zu of %zu bytes\n", offset, bits.size()); return 2; }
  std::vector<uint8_t> raw = slurp(dir + "/g19_pocsag_repair_in.bin");
  const size_t nw = raw.size() / 4;
  std::vector<uint32_t> out(2 * nw);
  for (size_t i = 0; i < nw; i++) {
    uint32_t w;
    memcpy(&w, &raw[4 * i], 4);
    out[2 * i] = (uint32_t)pocsag_repair(w);
    out[2 * i + 1] = w;
  }
  FILE *f = fopen((dir + "/g19_pocsag_repair_out.bin").c_str(), "wb");
  if (!f) { perror("g19_pocsag_repair_out.bin"); return 2; }
  fwrite(out.data(), 4, out.size(), f);
  fclose(f);
  js << "\n ],\n \"messages\": " << total_msgs << ",\n \"repair_in\": {\"file\": \"g19_pocsag_repair_in.bin\", \"dtype\": \"u32\", \"count\": " << nw
     << "},\n \"repair_out\": {\"file\": \"g19_pocsag_repair_out.bin\", \"dtype\": \"u32\", \"count\": " << 2 * nw << "}\n}\n";
  f = fopen((dir + "/manifest_pocsag.json").c_str(), "w");
  if (!f) { perror("manifest_pocsag.json"); return 2; }
  fputs(js.str().c_str(), f);
  fclose(f);
  return 0;
}

// `rows` nodes, one row of `n` bits each — what the decoder bank does in one call — on one core; the median of `reps` passes
static int bench(const std::string &path, size_t rows, size_t n, int reps) {
  std::vector<uint8_t> bits = slurp(path);
  if (bits.size() < rows * n) { fprintf(stderr, "%s: %zu bytes < %zu\n", path.c_str(), bits.size(), rows * n); return 2; }
  std::vector<double> ms;
  for (int r = -1; r < reps; r++) {
    std::vector<Feeder> src(rows);
    std::vector<Probe> node(rows);
    for (size_t c = 0; c < rows; c++) { src[c].connect(&node[c], true); src[c].configure(n); }
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    for (size_t c = 0; c < (r < 0 ? std::min<size_t>(rows, 16) : rows); c++) src[c].feed(bits.data() + c * n, n);
    const double dt = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (r >= 0) ms.push_back(dt);
  }
  std::sort(ms.begin(), ms.end());
  printf("{\"rows\": %zu, \"n\": %zu, \"reps\": %d, \"cpu_reference_ms\": %.3f, \"min_ms\": %.3f, \"max_ms\": %.3f}\n", rows, n, reps,
         ms[ms.size() / 2], ms.front(), ms.back());
  return 0;
}

int main(int argc, char **argv) {
  if (argc >= 3 && std::string(argv[1]) == "golden") return golden(argv[2]);
  if (argc >= 5 && std::string(argv[1]) == "bench") return bench(argv[2], strtoul(argv[3], 0, 10), strtoul(argv[4], 0, 10), 3);
  fprintf(stderr, "usage: cut golden <dir> | cut bench <rows.bin> <rows> <bits>\n");
  return 1;
}
