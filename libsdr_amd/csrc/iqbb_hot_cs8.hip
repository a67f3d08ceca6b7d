// iqbb_hot_cs8.hip — the hot kernel (iqbb_hot.hpp): the /8 form, complex<int8> (one unit per class group: they compile in parallel)
#define SDRHIP_HOT_INSTANTIATE
#include "iqbb_hot.hpp"
template struct sdrhip::HotClass<HOT_D8, 2, HOT_CS8>; template struct sdrhip::HotClass<HOT_D8, 3, HOT_CS8>;
template struct sdrhip::HotClass<HOT_D8, 5, HOT_CS8>; template struct sdrhip::HotClass<HOT_D8, 9, HOT_CS8>;
