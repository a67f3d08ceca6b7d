// iqbb_hot_real.hip — the hot kernel (iqbb_hot.hpp): the /8 form, real input, 3 and 5 K steps (one unit per class group: they compile in parallel)
#define SDRHIP_HOT_INSTANTIATE
#include "iqbb_hot.hpp"
template struct sdrhip::HotClass<HOT_D8, 3, HOT_REAL>; template struct sdrhip::HotClass<HOT_D8, 5, HOT_REAL>;
