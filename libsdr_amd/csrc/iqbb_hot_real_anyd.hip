// iqbb_hot_real_anyd.hip — the hot kernel (iqbb_hot.hpp): the any-D form, real input, 3 and 5 K steps (one unit per class group: they compile in parallel)
#define SDRHIP_HOT_INSTANTIATE
#include "iqbb_hot.hpp"
template struct sdrhip::HotClass<HOT_ANYD, 3, HOT_REAL>; template struct sdrhip::HotClass<HOT_ANYD, 5, HOT_REAL>;
