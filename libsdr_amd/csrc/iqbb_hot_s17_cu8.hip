// iqbb_hot_s17_cu8.hip — the hot kernel (iqbb_hot.hpp): the /8 form, 17 K steps (orders up to 257), complex<uint8> (one unit per class group: they compile in parallel)
#define SDRHIP_HOT_INSTANTIATE
#include "iqbb_hot.hpp"
template struct sdrhip::HotClass<HOT_D8, 17, HOT_CU8>;
