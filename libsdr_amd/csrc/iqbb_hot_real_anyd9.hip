// iqbb_hot_real_anyd9.hip — the hot kernel (iqbb_hot.hpp): the any-D form, real input, 9 K steps (one unit per class group: they compile in parallel)
#define SDRHIP_HOT_INSTANTIATE
#include "iqbb_hot.hpp"
template struct sdrhip::HotClass<HOT_ANYD, 9, HOT_REAL>;
