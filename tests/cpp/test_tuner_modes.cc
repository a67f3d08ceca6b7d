// test_tuner_modes.cc — sdr::gpu::TunerBank<int16_t> with a demodulator per channel (TunerBank::PerChannel,
// include/sdr/gpu/nodes.hh): IQSigGen -> bank -> one Recorder per channel, against three banks with ONE demodulator each on the
// same source, and setMode() between buffers.
//   test_tuner_modes --host-only   what needs no device: modes recorded before config(), mode(c), ConfigError (built under ASan/UBSan)
//   test_tuner_modes               + the graphs on the GPU
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "sdr/sdr.hh"

using namespace sdr;
typedef std::complex<int16_t> cs16;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

static const double FS = 2.4e6;
static const size_t BS = 4096;

struct TuneSpec { double Fc, Ff, width; int mode; };
// NFM, an AM channel beside it, USB (the filter 1500 Hz above the carrier: examples/sdr_rec.cc:53-55 of the reference)
static const TuneSpec TUNES[] = {{100e3, 100e3, 12.5e3, SDRHIP_EPI_FM}, {-300e3, -300e3, 15e3, SDRHIP_EPI_AM}, {210e3, 211.5e3, 3e3, SDRHIP_EPI_USB}};
static const size_t NT = 3;
static const int MODES[] = {SDRHIP_EPI_FM, SDRHIP_EPI_AM, SDRHIP_EPI_USB};

template <class F> static bool throwsConfigError(F f) {
  try { f(); } catch (ConfigError &) { return true; }
  return false;
}

static void testHostOnly() {
  gpu::TunerBank<int16_t> bank(127, 8, gpu::TunerBank<int16_t>::PerChannel);
  CHECK(bank.perChannel());
  CHECK(bank.addChannel(100e3, 100e3, 12.5e3) == 0 && bank.mode(0) == SDRHIP_EPI_FM);   // the default of a per-channel bank
  CHECK(bank.addChannel(-300e3, -300e3, 15e3, SDRHIP_EPI_AM) == 1 && bank.mode(1) == SDRHIP_EPI_AM);
  CHECK(bank.addChannel(210e3, 211.5e3, 3e3, SDRHIP_EPI_USB) == 2 && bank.mode(2) == SDRHIP_EPI_USB);
  bank.setMode(0, SDRHIP_EPI_USB); bank.setMode(2, SDRHIP_EPI_FM);                     // before config(): recorded
  CHECK(bank.mode(0) == SDRHIP_EPI_USB && bank.mode(1) == SDRHIP_EPI_AM && bank.mode(2) == SDRHIP_EPI_FM);
  // what a per-channel bank has no demodulator for: nothing changes
  CHECK(throwsConfigError([&] { bank.setMode(1, SDRHIP_EPI_NONE); }) && throwsConfigError([&] { bank.setMode(1, 7); }));
  CHECK(throwsConfigError([&] { bank.addChannel(0, 0, 10e3, SDRHIP_EPI_NONE); }));
  CHECK(bank.channels() == 3 && bank.mode(1) == SDRHIP_EPI_AM);
  // a bank with one demodulator for all: its own mode is accepted, any other throws
  gpu::TunerBank<int16_t> am(127, 8, SDRHIP_EPI_AM), raw(21, 8);
  CHECK(!am.perChannel() && am.addChannel(0, 0, 15e3) == 0 && am.addChannel(1e3, 1e3, 15e3, SDRHIP_EPI_AM) == 1);
  CHECK(am.mode(0) == SDRHIP_EPI_AM && am.mode(1) == SDRHIP_EPI_AM);
  am.setMode(1, SDRHIP_EPI_AM);
  CHECK(throwsConfigError([&] { am.setMode(1, SDRHIP_EPI_FM); }) && throwsConfigError([&] { am.addChannel(0, 0, 15e3, SDRHIP_EPI_USB); }));
  CHECK(am.channels() == 2 && am.mode(1) == SDRHIP_EPI_AM);
  CHECK(raw.addChannel(0, 0, 15e3) == 0 && raw.mode(0) == SDRHIP_EPI_NONE && throwsConfigError([&] { raw.setMode(0, SDRHIP_EPI_FM); }));
  // with a complete Config: a plan or a ConfigError (no device, no CPU fallback), never a crash
  try { bank.config(Config(Config::Type_cs16, FS, BS, 1)); } catch (ConfigError &e) { (void)e; }
}

static void testMixedAgainstSingleBanks() {
  const size_t NB = 4;
  IQSigGen<int16_t> gen(FS, BS);
  gen.addSine(100e3, 8000, 0.0); gen.addSine(-300e3, 6000, 0.3); gen.addSine(211e3, 7000, 1.0);
  gpu::TunerBank<int16_t> mixed(127, 8, gpu::TunerBank<int16_t>::PerChannel);
  gpu::TunerBank<int16_t> fm(127, 8, SDRHIP_EPI_FM), amb(127, 8, SDRHIP_EPI_AM), usb(127, 8, SDRHIP_EPI_USB);
  gpu::TunerBank<int16_t> *single[] = {&fm, &amb, &usb};      // (indexed as MODES)
  std::vector<Recorder<int16_t> > out(NT);
  std::vector<std::vector<Recorder<int16_t> > > ref(3, std::vector<Recorder<int16_t> >(NT));
  for (size_t c = 0; c < NT; c++) {
    CHECK(mixed.addChannel(TUNES[c].Fc, TUNES[c].Ff, TUNES[c].width, TUNES[c].mode) == c);
    for (size_t m = 0; m < 3; m++) single[m]->addChannel(TUNES[c].Fc, TUNES[c].Ff, TUNES[c].width);
  }
  gen.connect(&mixed, true);
  for (size_t m = 0; m < 3; m++) gen.connect(single[m], true);
  for (size_t c = 0; c < NT; c++) {
    mixed.source(c)->connect(&out[c], true);
    for (size_t m = 0; m < 3; m++) single[m]->source(c)->connect(&ref[m][c], true);
    CHECK(mixed.source(c)->type() == Config::Type_s16 && mixed.source(c)->sampleRate() == 300000.0);   // int16_t at the same rate
  }
  // per buffer and source: where the output starts
  std::vector<std::vector<size_t> > at(NB + 1, std::vector<size_t>(NT, 0));
  for (size_t b = 0; b < NB; b++) {
    if (b == 2) {   // after buffer 2: a new FMDemod behind channel 1's baseband
      CHECK(mixed.mode(1) == SDRHIP_EPI_AM);
      mixed.setMode(1, SDRHIP_EPI_FM);
      CHECK(mixed.mode(1) == SDRHIP_EPI_FM);
    }
    gen.next();
    for (size_t c = 0; c < NT; c++) at[b + 1][c] = out[c].data.size();
  }
  const size_t lens[] = {511, 512, 512, 512};
  for (size_t c = 0; c < NT; c++) {
    CHECK(out[c].lens == std::vector<size_t>(lens, lens + NB));
    for (size_t m = 0; m < 3; m++) CHECK(ref[m][c].data.size() == out[c].data.size());
  }
  if (failures) return;
  auto same = [&](size_t c, size_t m, size_t lo, size_t hi) {
    return std::vector<int16_t>(out[c].data.begin() + lo, out[c].data.begin() + hi) ==
           std::vector<int16_t>(ref[m][c].data.begin() + lo, ref[m][c].data.begin() + hi);
  };
  // sources 0 and 2: the single-demodulator bank of their mode, all four buffers — the switch of channel 1 changed nothing
  CHECK(same(0, 0, 0, at[NB][0]) && same(2, 2, 0, at[NB][2]));
  CHECK(!same(0, 1, 0, at[NB][0]) && !same(2, 0, 0, at[NB][2]));     // (the modes do differ on this signal)
  // source 1: AM for two buffers; then FM from a fresh FMDemod: out[0] in place, out[1] against angle 0 instead of the FM
  // bank's carried angle, everything behind it equal to the FM bank's row
  CHECK(same(1, 1, 0, at[2][1]) && !same(1, 1, at[2][1], at[NB][1]));
  CHECK(same(1, 0, at[2][1], at[2][1] + 1) && same(1, 0, at[2][1] + 2, at[NB][1]));
  CHECK(out[1].data[at[2][1] + 1] != ref[0][1].data[at[2][1] + 1]);
  // a mode the bank has no demodulator for leaves the running plan as it is
  CHECK(throwsConfigError([&] { mixed.setMode(0, SDRHIP_EPI_NONE); }) && mixed.mode(0) == SDRHIP_EPI_FM);
  CHECK(throwsConfigError([&] { fm.setMode(0, SDRHIP_EPI_AM); }));
}

int main(int argc, char **argv) {
  const bool host_only = argc > 1 && std::string(argv[1]) == "--host-only";
  Logger::get().addHandler(new StreamLogHandler(std::cerr, LOG_ERROR));
  try {
    testHostOnly();
    if (!host_only) testMixedAgainstSingleBanks();
  } catch (std::exception &e) { std::printf("FAIL: exception: %s\n", e.what()); return 2; }
  std::printf("%s (%d failures)\n", failures ? "FAILED" : "OK", failures);
  return failures ? 1 : 0;
}
