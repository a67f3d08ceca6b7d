// iqbb_hot_sd9.hip — the hot kernel (iqbb_hot.hpp): the small-D form, 9 K steps (one unit per class group: they compile in parallel)
#define SDRHIP_HOT_INSTANTIATE
#include "iqbb_hot.hpp"
template struct sdrhip::HotClass<HOT_SD, 9, HOT_CS16>; template struct sdrhip::HotClass<HOT_SD, 9, HOT_CU8>;
