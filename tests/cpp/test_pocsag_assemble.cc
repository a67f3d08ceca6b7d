// test_pocsag_assemble.cc — the C++ message assembly (include/sdr/gpu/pocsag_message.hh) alone: no HIP, no library. Feeds the
// golden cases' event streams to pocsag::Assembler and compares what it releases at every END with what the reference
// delivered there. Built with -fsanitize=address,undefined by tests/test_cpp_pocsag_assemble.py.
//   test_pocsag_assemble <cases.txt>
#include "pocsag_cases.hh"

using namespace sdr::gpu;

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: test_pocsag_assemble <cases.txt>\n"); return 2; }
  const std::vector<cases::Case> all = cases::load(argv[1]);
  int failures = 0;
  size_t messages = 0, ends = 0;
  for (size_t i = 0; i < all.size(); i++) {
    const cases::Case &c = all[i];
    pocsag::Assembler a;
    size_t next = 0;
    bool released = false;
    for (size_t k = 0; k < c.items.size(); k++) {
      const cases::Item &it = c.items[k];
      if (it.isEvent) {
        if (released) { printf("FAIL %s: an END with no delivery recorded behind it\n", c.name.c_str()); failures++; a.queue().clear(); }
        released = a.feed(it.word, it.info);
        ends += released;
        continue;
      }
      if (!released) { printf("FAIL %s: delivery %zu expected, but the last event released nothing\n", c.name.c_str(), next); failures++; }
      released = false;
      const cases::Delivery &d = c.deliveries[next++];
      if (a.queue().size() != d.msgs.size()) {
        printf("FAIL %s: delivery %zu has %zu messages, want %zu\n", c.name.c_str(), next - 1, a.queue().size(), d.msgs.size());
        failures++;
      } else
        for (size_t m = 0; m < d.msgs.size(); m++, messages++) failures += cases::differs(c.name.c_str(), a.queue()[m], d.msgs[m]);
      a.queue().clear();
    }
    if (released || next != c.deliveries.size()) { printf("FAIL %s: %zu of %zu deliveries seen\n", c.name.c_str(), next, c.deliveries.size()); failures++; }
  }
  // the readings of an empty and of a partly filled message do not look beyond the payload
  pocsag::Message none, open(0x1234u << 3 | 5u, 2);
  if (!none.isEmpty() || open.isEmpty() || open.address() != ((0x1234u << 3) | 5u) || !open.asText().empty() || !open.asNumeric().empty() ||
      open.estimateText() != 0 || open.estimateNumeric() != 0) { printf("FAIL: empty messages\n"); failures++; }
  open.addPayload(0x80000000u | (0xABCDEu << 11));
  if (open.bits() != 20 || open.payload().size() != 3 || open.payload()[0] != 0xAB || open.payload()[1] != 0xCD || open.payload()[2] != 0x0E ||
      open.asNumeric().size() != 5 || open.asText().size() < 2) { printf("FAIL: one data word\n"); failures++; }
  if (all.size() < 10 || messages < 20 || ends < 15) { printf("FAIL: the case file is thin (%zu cases, %zu messages, %zu ENDs)\n", all.size(), messages, ends); failures++; }
  printf("%zu cases, %zu messages, %zu ENDs\nOK (%d failures)\n", all.size(), messages, ends, failures);
  return failures ? 1 : 0;
}
