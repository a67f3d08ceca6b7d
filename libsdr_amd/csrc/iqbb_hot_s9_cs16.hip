// iqbb_hot_s9_cs16.hip — explicit instantiations of the hot kernel (iqbb_hot.hpp) for S = 9 K steps (orders up to 129), complex<int16> input; one translation unit per filter-length
// class so that the build compiles them in parallel.
#include "iqbb_hot.hpp"

namespace sdrhip {
// lo = 0: the low-plane range [1, 8) of hot_lo_ranges_9 — every high-plane range but the full one lies inside it (the host
// never pairs it with that one); lo = 1: all 9 steps
void hot_launch_s9_cs16(int range, int lo, bool rot, int epi, const HotLaunch &hl, const HotArgs &ha, const IqbbArgs &b) {
  if (lo == 0 && range <= 2) {
    switch (range) {
      case 0: hot_launch_one<9, 3, 3, HOT_CS16, 4, 1, 7>(rot, epi, hl, ha, b); break;
      case 1: hot_launch_one<9, 2, 5, HOT_CS16, 4, 1, 7>(rot, epi, hl, ha, b); break;
      default: hot_launch_one<9, 1, 7, HOT_CS16, 4, 1, 7>(rot, epi, hl, ha, b); break;
    }
    return;
  }
  switch (range) {
    case 0: hot_launch_one<9, 3, 3, HOT_CS16, 4>(rot, epi, hl, ha, b); break;
    case 1: hot_launch_one<9, 2, 5, HOT_CS16, 4>(rot, epi, hl, ha, b); break;
    case 2: hot_launch_one<9, 1, 7, HOT_CS16, 4>(rot, epi, hl, ha, b); break;
    default: hot_launch_one<9, 0, 9, HOT_CS16, 4>(rot, epi, hl, ha, b); break;
  }
}
}  // namespace sdrhip
