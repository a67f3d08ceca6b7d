// iqbb_hot_anyd9.hip — the hot kernel (iqbb_hot.hpp): the any-D form, 9 K steps (one unit per class group: they compile in parallel)
#define SDRHIP_HOT_INSTANTIATE
#include "iqbb_hot.hpp"
template struct sdrhip::HotClass<HOT_ANYD, 9, HOT_CS16>; template struct sdrhip::HotClass<HOT_ANYD, 9, HOT_CU8>;
