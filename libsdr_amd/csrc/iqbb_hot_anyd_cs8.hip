// iqbb_hot_anyd_cs8.hip — the hot kernel (iqbb_hot.hpp): the any-D form, complex<int8> (one unit per class group: they compile in parallel)
#define SDRHIP_HOT_INSTANTIATE
#include "iqbb_hot.hpp"
template struct sdrhip::HotClass<HOT_ANYD, 2, HOT_CS8>; template struct sdrhip::HotClass<HOT_ANYD, 3, HOT_CS8>;
template struct sdrhip::HotClass<HOT_ANYD, 5, HOT_CS8>; template struct sdrhip::HotClass<HOT_ANYD, 9, HOT_CS8>;
