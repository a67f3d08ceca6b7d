// iqbb_hot_real9.hip — the hot kernel (iqbb_hot.hpp): the /8 form, real input, 9 K steps (one unit per class group: they compile in parallel)
#define SDRHIP_HOT_INSTANTIATE
#include "iqbb_hot.hpp"
template struct sdrhip::HotClass<HOT_D8, 9, HOT_REAL>;
