// iqbb_hot_s17_cs16.hip — the hot kernel (iqbb_hot.hpp): the /8 form, 17 K steps (orders up to 257), complex<int16> (one unit per class group: they compile in parallel)
#define SDRHIP_HOT_INSTANTIATE
#include "iqbb_hot.hpp"
template struct sdrhip::HotClass<HOT_D8, 17, HOT_CS16>;
