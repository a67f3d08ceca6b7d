// iqbb_hot_real_sd.hip — the hot kernel (iqbb_hot.hpp): the small-D form, real input, 3 and 5 K steps (one unit per class group: they compile in parallel)
#define SDRHIP_HOT_INSTANTIATE
#include "iqbb_hot.hpp"
template struct sdrhip::HotClass<HOT_SD, 3, HOT_REAL>; template struct sdrhip::HotClass<HOT_SD, 5, HOT_REAL>;
