// Winograd-domain conv, several convs per launch (conv1d_wino.h: conv1d_wino_multi_kernel): the K = 11, 7 and 3 bodies of
// one (dilation, rows per workgroup) family in one persistent kernel -- 128-row and 64-row workgroups, dilations 1, 3, 5,
// two fragments per wave.
#include "conv1d_wino.h"

int ovkw::wino_multi_dispatch(const wino_multi_args* a, int nwg, hipStream_t st) {
  const ov_conv1d_wino_params* p = &a->seg[(a->present & 1) ? 0 : ((a->present & 2) ? 1 : 2)];
  const int mw = wino_mw(p->Cout);
  if (mw == 4) {
    if (p->dil == 1) return wino_multi_launch<1, 2, 4>(a, nwg, st);
    if (p->dil == 3) return wino_multi_launch<3, 2, 4>(a, nwg, st);
    if (p->dil == 5) return wino_multi_launch<5, 2, 4>(a, nwg, st);
  } else if (mw == 2) {
    if (p->dil == 1) return wino_multi_launch<1, 2, 2>(a, nwg, st);
    if (p->dil == 3) return wino_multi_launch<3, 2, 2>(a, nwg, st);
    if (p->dil == 5) return wino_multi_launch<5, 2, 2>(a, nwg, st);
  }
  return OV_E_UNSUPPORTED;
}
