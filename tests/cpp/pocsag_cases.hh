// pocsag_cases.hh — TEST CODE: reads the case file tests/test_cpp_pocsag*.py write from the golden fixtures
// (tests/golden/manifest_pocsag.json) for the two C++ programs. Whitespace-separated tokens:
//   c <name>                                   a new case
//   e <word> <info>                            an event, in order (from the restatement; the assembly test feeds them)
//   d <call>                                   the reference delivered its queue here (after the END just before), in call <call>
//   m <address> <function> <bits> <payload hex|-> <estimateText> <estimateNumeric> <asNumeric hex|-> <asText hex|->
#pragma once
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "sdr/gpu/pocsag_message.hh"

namespace cases {

struct Msg { uint32_t address; unsigned function, bits; std::vector<uint8_t> payload; int estText, estNum; std::string numeric, text; };
struct Delivery { int call; std::vector<Msg> msgs; };
struct Item { bool isEvent; uint32_t word, info; };   // an event, or (isEvent false) "the next delivery belongs here"
struct Case { std::string name; std::vector<Item> items; std::vector<Delivery> deliveries; };

inline std::vector<uint8_t> unhex(const std::string &s) {
  std::vector<uint8_t> v;
  if (s == "-") return v;
  for (size_t i = 0; i + 1 < s.size(); i += 2) v.push_back(uint8_t(std::stoul(s.substr(i, 2), 0, 16)));
  return v;
}

inline std::vector<Case> load(const char *path) {
  std::vector<Case> out;
  std::ifstream f(path);
  std::string tok;
  while (f >> tok) {
    if (tok == "c") { out.push_back(Case()); f >> out.back().name; }
    else if (tok == "e") { Item it = {true, 0, 0}; f >> it.word >> it.info; out.back().items.push_back(it); }
    else if (tok == "d") { Delivery d; f >> d.call; out.back().deliveries.push_back(d); Item it = {false, 0, 0}; out.back().items.push_back(it); }
    else if (tok == "m") {
      Msg m; std::string p, n, t;
      f >> m.address >> m.function >> m.bits >> p >> m.estText >> m.estNum >> n >> t;
      m.payload = unhex(p);
      std::vector<uint8_t> nv = unhex(n), tv = unhex(t);
      m.numeric.assign(nv.begin(), nv.end()); m.text.assign(tv.begin(), tv.end());
      out.back().deliveries.back().msgs.push_back(m);
    }
  }
  return out;
}

// 0 when `got` is the message the reference delivered, in every field and reading; prints what differs
inline int differs(const char *where, const sdr::gpu::pocsag::Message &got, const Msg &want) {
  const bool same = got.address() == want.address && got.function() == want.function && got.bits() == want.bits &&
                    got.payload() == want.payload && got.estimateText() == want.estText && got.estimateNumeric() == want.estNum &&
                    got.asNumeric() == want.numeric && got.asText() == want.text;
  if (!same)
    printf("FAIL %s: got @%u F%u bits %u est %d/%d num '%s' text '%s', want @%u F%u bits %u est %d/%d num '%s' text '%s'\n", where,
           got.address(), unsigned(got.function()), got.bits(), got.estimateText(), got.estimateNumeric(), got.asNumeric().c_str(),
           got.asText().c_str(), want.address, want.function, want.bits, want.estText, want.estNum, want.numeric.c_str(), want.text.c_str());
  return same ? 0 : 1;
}

}  // namespace cases
