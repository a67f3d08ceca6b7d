// iqbb_hot_anyd17_cs16.hip — the hot kernel (iqbb_hot.hpp): the any-D form, 17 K steps, complex<int16> (one unit per class group: they compile in parallel)
#define SDRHIP_HOT_INSTANTIATE
#include "iqbb_hot.hpp"
template struct sdrhip::HotClass<HOT_ANYD, 17, HOT_CS16>;
