// iqbb_hot_sd17_cs16.hip — the hot kernel (iqbb_hot.hpp): the small-D form, 17 K steps, complex<int16> (one unit per class group: they compile in parallel)
#define SDRHIP_HOT_INSTANTIATE
#include "iqbb_hot.hpp"
template struct sdrhip::HotClass<HOT_SD, 17, HOT_CS16>;
