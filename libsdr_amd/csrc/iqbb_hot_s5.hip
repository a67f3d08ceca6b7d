// iqbb_hot_s5.hip — the hot kernel (iqbb_hot.hpp): the /8 form, 5 K steps (orders up to 65) (one unit per class group: they compile in parallel)
#define SDRHIP_HOT_INSTANTIATE
#include "iqbb_hot.hpp"
template struct sdrhip::HotClass<HOT_D8, 5, HOT_CS16>; template struct sdrhip::HotClass<HOT_D8, 5, HOT_CU8>;
