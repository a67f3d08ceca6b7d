// iqbb_hot_s9_cs16.hip — the hot kernel (iqbb_hot.hpp): the /8 form, 9 K steps (orders up to 129), complex<int16> (one unit per class group: they compile in parallel)
#define SDRHIP_HOT_INSTANTIATE
#include "iqbb_hot.hpp"
template struct sdrhip::HotClass<HOT_D8, 9, HOT_CS16>;
