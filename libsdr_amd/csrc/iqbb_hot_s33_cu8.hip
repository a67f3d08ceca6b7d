// iqbb_hot_s33_cu8.hip — the hot kernel (iqbb_hot.hpp): the /8 form, 33 K steps (orders up to 513), complex<uint8> (one unit per class group: they compile in parallel)
#define SDRHIP_HOT_INSTANTIATE
#include "iqbb_hot.hpp"
template struct sdrhip::HotClass<HOT_D8, 33, HOT_CU8>;
