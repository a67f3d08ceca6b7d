// iqbb_hot_s3.hip — the hot kernel (iqbb_hot.hpp): the /8 form, 3 K steps (orders up to 33) (one unit per class group: they compile in parallel)
#define SDRHIP_HOT_INSTANTIATE
#include "iqbb_hot.hpp"
template struct sdrhip::HotClass<HOT_D8, 3, HOT_CS16>; template struct sdrhip::HotClass<HOT_D8, 3, HOT_CU8>;
