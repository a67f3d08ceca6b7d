// test_pocsag_bank.cc — sdr::gpu::POCSAGBank (include/sdr/gpu/pocsag.hh) on the GPU: every golden row is one channel of ONE
// bank, fed in its recorded call splits (call k gives row c its k-th split, 0 bits once the row is used up) through the
// host-row process() and, from a device copy of the same rows, through processDev() on a second bank. handleMessages(channel)
// has to deliver, per channel, the reference's deliveries: the same calls, the same messages.
//   test_pocsag_bank <cases.txt> <g19_pocsag_inputs.txt> <g19_pocsag_bits.bin>
#include <algorithm>
#include <iterator>
#include <memory>

#include "sdr/gpu/pocsag.hh"
#include "pocsag_cases.hh"

using namespace sdr;

struct Row { std::string name; size_t offset, n; std::vector<size_t> splits; };

class Recorder : public gpu::POCSAGBank {
public:
  Recorder(size_t channels, size_t maxBits) : gpu::POCSAGBank(channels, maxBits), call(0), got(channels) {}
  int call;
  std::vector<std::vector<std::pair<int, std::vector<Message> > > > got;
  virtual void handleMessages(size_t c) {
    got[c].push_back(std::make_pair(call, queue(c)));
    queue(c).clear();
  }
};

static int compare(const char *what, const std::vector<cases::Case> &want, const Recorder &bank) {
  int failures = 0;
  size_t messages = 0;
  for (size_t c = 0; c < want.size(); c++) {
    const std::vector<cases::Delivery> &w = want[c].deliveries;
    if (bank.got[c].size() != w.size()) {
      printf("FAIL %s %s: %zu deliveries, want %zu\n", what, want[c].name.c_str(), bank.got[c].size(), w.size());
      failures++;
      continue;
    }
    for (size_t d = 0; d < w.size(); d++) {
      if (bank.got[c][d].first != w[d].call || bank.got[c][d].second.size() != w[d].msgs.size()) {
        printf("FAIL %s %s: delivery %zu in call %d with %zu messages, want call %d with %zu\n", what, want[c].name.c_str(), d,
               bank.got[c][d].first, bank.got[c][d].second.size(), w[d].call, w[d].msgs.size());
        failures++;
        continue;
      }
      for (size_t m = 0; m < w[d].msgs.size(); m++, messages++) failures += cases::differs(want[c].name.c_str(), bank.got[c][d].second[m], w[d].msgs[m]);
    }
  }
  if (messages < 20) { printf("FAIL %s: only %zu messages compared\n", what, messages); failures++; }
  printf("%s: %zu channels, %zu messages\n", what, want.size(), messages);
  return failures;
}

int main(int argc, char **argv) {
  if (argc < 4) { fprintf(stderr, "usage: test_pocsag_bank <cases.txt> <inputs.txt> <bits.bin>\n"); return 2; }
  const std::vector<cases::Case> want = cases::load(argv[1]);
  std::vector<Row> rows;
  {
    std::ifstream f(argv[2]);
    Row r;
    size_t ns, offset = 0;
    while (f >> r.name >> r.n >> ns) {
      r.splits.resize(ns);
      for (size_t i = 0; i < ns; i++) f >> r.splits[i];
      r.offset = offset;
      offset += r.n;
      rows.push_back(r);
    }
  }
  std::ifstream fb(argv[3], std::ios::binary);
  const std::vector<uint8_t> bits((std::istreambuf_iterator<char>(fb)), std::istreambuf_iterator<char>());
  int failures = 0;
  if (rows.size() != want.size() || rows.empty() || bits.size() != rows.back().offset + rows.back().n) {
    printf("FAIL: %zu rows, %zu cases, %zu bytes\n", rows.size(), want.size(), bits.size());
    printf("OK (1 failures)\n");
    return 1;
  }
  const size_t C = rows.size(), maxBits = 2048, stride = maxBits + 7;
  size_t calls = 0;
  for (size_t c = 0; c < C; c++) {
    calls = std::max(calls, rows[c].splits.size());
    if (rows[c].name != want[c].name) { printf("FAIL: row %zu is %s, case %s\n", c, rows[c].name.c_str(), want[c].name.c_str()); failures++; }
  }
  try {
    Recorder host(C, maxBits), dev(C, maxBits);
    sdrhip_ctx *ctx = gpu::Device::get(0);
    gpu::detail::DeviceMem dbits, dcounts;
    dbits.alloc(ctx, C * stride, "test");
    dcounts.alloc(ctx, C * sizeof(uint32_t), "test");
    std::vector<uint8_t> buf(C * stride);
    std::vector<uint32_t> counts(C);
    std::vector<size_t> at(C, 0);
    for (size_t k = 0; k < calls; k++) {
      std::fill(buf.begin(), buf.end(), uint8_t(0xA5));   // bit 0 set behind every count
      for (size_t c = 0; c < C; c++) {
        counts[c] = k < rows[c].splits.size() ? uint32_t(rows[c].splits[k]) : 0;
        std::copy(bits.begin() + rows[c].offset + at[c], bits.begin() + rows[c].offset + at[c] + counts[c], buf.begin() + c * stride);
        at[c] += counts[c];
      }
      host.call = dev.call = int(k);
      if (!host.process(buf.data(), stride, counts.data())) { printf("FAIL: process, call %zu\n", k); failures++; }
      gpu::detail::configCheck(sdrhip_memcpy_h2d_async(ctx, dbits.get(), buf.data(), buf.size()), "test");
      gpu::detail::configCheck(sdrhip_memcpy_h2d_async(ctx, dcounts.get(), counts.data(), C * sizeof(uint32_t)), "test");
      if (!dev.processDev(dbits.as<uint8_t>(), stride, dcounts.as<uint32_t>())) { printf("FAIL: processDev, call %zu\n", k); failures++; }
    }
    failures += compare("process", want, host);
    failures += compare("processDev", want, dev);
    // a reset bank is a fresh one: the first row again, in one call, delivers its first delivery again
    host.reset();
    host.got.assign(C, std::vector<std::pair<int, std::vector<gpu::POCSAGBank::Message> > >());
    std::fill(counts.begin(), counts.end(), 0u);
    counts[0] = uint32_t(rows[0].n);
    std::copy(bits.begin(), bits.begin() + rows[0].n, buf.begin());
    host.call = 0;
    host.process(buf.data(), stride, counts.data());
    if (host.got[0].size() != want[0].deliveries.size() || host.got[0].empty() || host.got[0][0].second.size() != want[0].deliveries[0].msgs.size()) {
      printf("FAIL: after reset\n");
      failures++;
    }
  } catch (const std::exception &e) {
    printf("FAIL: exception: %s\n", e.what());
    failures++;
  }
  printf("OK (%d failures)\n", failures);
  return failures ? 1 : 0;
}
