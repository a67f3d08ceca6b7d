// iqbb_hot_anyd.hip — the hot kernel (iqbb_hot.hpp): the any-D form, 2, 3 and 5 K steps (one unit per class group: they compile in parallel)
#define SDRHIP_HOT_INSTANTIATE
#include "iqbb_hot.hpp"
template struct sdrhip::HotClass<HOT_ANYD, 2, HOT_CS16>; template struct sdrhip::HotClass<HOT_ANYD, 2, HOT_CU8>;
template struct sdrhip::HotClass<HOT_ANYD, 3, HOT_CS16>; template struct sdrhip::HotClass<HOT_ANYD, 3, HOT_CU8>;
template struct sdrhip::HotClass<HOT_ANYD, 5, HOT_CS16>; template struct sdrhip::HotClass<HOT_ANYD, 5, HOT_CU8>;
