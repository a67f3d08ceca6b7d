// iqbb_hot_anyd17_cu8.hip — the hot kernel (iqbb_hot.hpp): the any-D form, 17 K steps, complex<uint8> (one unit per class group: they compile in parallel)
#define SDRHIP_HOT_INSTANTIATE
#include "iqbb_hot.hpp"
template struct sdrhip::HotClass<HOT_ANYD, 17, HOT_CU8>;
