// Panel GEMM, FairLoRA epilogues: the row of unit 3, the 208x384 tile with two waves per SIMD.  See gemm_panel_rk.hip.
#include "gemm_panel_impl.h"

int ffm_panel_launch_rk3(const ffm_gemm_args& a, int cfg, hipStream_t s) { return ffm_panel::launch_unit<3>(a, cfg, s); }
