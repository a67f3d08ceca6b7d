// harness.hh — what the node test programs of this directory share: a binary file reader, a Source that feeds views of the
// caller's samples, a Sink that keeps what it is sent, the "this construction throws ConfigError" probe of the rules modes and
// the wrapper of main (an SDRError is one more failure; the last line is "OK (0 failures)" or "FAILED (n failures)").
#ifndef SDR_TESTS_CPP_HARNESS_HH
#define SDR_TESTS_CPP_HARNESS_HH

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "sdr/gpu/nodes.hh"

using namespace sdr;

template <class T>
static std::vector<T> readBin(const std::string &path, size_t count) {
  std::vector<T> v(count);
  std::ifstream f(path.c_str(), std::ios::binary);
  f.read(reinterpret_cast<char *>(v.data()), count * sizeof(T));
  if ((size_t)f.gcount() != count * sizeof(T)) { fprintf(stderr, "%s: short file\n", path.c_str()); exit(2); }
  return v;
}

template <class T>
class Capture : public Sink<T> {
public:
  std::vector<T> data;
  Config cfg;
  virtual void config(const Config &c) { cfg = c; }
  virtual void process(const Buffer<T> &b, bool) {
    for (size_t i = 0; i < b.size(); i++) data.push_back(b[i]);
  }
};

template <class T>
class Feeder : public Source {
public:
  void configure(double Fs, size_t maxlen) { this->setConfig(Config(Config::typeId<T>(), Fs, maxlen, 1)); }
  void feed(T *p, size_t n) { Buffer<T> view(p, n); this->send(view, false); }
};

template <class F>
static bool refused(F make) {
  try { make(); } catch (ConfigError &) { return true; } catch (SDRError &) {}
  return false;
}

// run(): the failures of the mode the arguments name, or -1 where they name none (the usage line, exit status 2)
template <class Run>
static int runMain(const char *usage, Run run) {
  int failures = 0;
  try {
    failures = run();
    if (failures < 0) { fprintf(stderr, "%s", usage); return 2; }
  } catch (SDRError &e) {
    printf("FAIL exception: %s\n", e.what());
    failures++;
  }
  printf("%s (%d failures)\n", failures ? "FAILED" : "OK", failures);
  return failures ? 1 : 0;
}

#endif
