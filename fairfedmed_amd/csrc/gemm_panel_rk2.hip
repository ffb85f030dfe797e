// Panel GEMM, FairLoRA epilogues: the rows of unit 2, the 160x128 tiles (4 waves; 8 waves as 4 column slabs x 2 K halves).
// See gemm_panel_rk.hip.
#include "gemm_panel_impl.h"

int ffm_panel_launch_rk2(const ffm_gemm_args& a, int cfg, hipStream_t s) { return ffm_panel::launch_unit<2>(a, cfg, s); }
