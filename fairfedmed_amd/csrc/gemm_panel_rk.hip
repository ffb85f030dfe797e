// Panel GEMM, FairLoRA epilogues (FFM_EPI_RANKOP): c_fc / c_proj forward and their dX products.
// The instantiations are split over three translation units so that they compile side by side: one unit took 6.5
// minutes.  Which unit has which row is the row's `unit` in FFM_PANEL_CFGS (gemm_panel.h): 1 is this file (the one-wave-
// per-SIMD 208x384 and 176x128 tiles), 2 gemm_panel_rk2.hip (the 160x128 tiles, 4 waves and the 8-wave K split), 3
// gemm_panel_rk3.hip (the 8-wave 208x384 tile).  Which epilogues a row has is ffm_panel_has.
#include "gemm_panel_impl.h"

int ffm_panel_launch_rk2(const ffm_gemm_args& a, int cfg, hipStream_t s);      // gemm_panel_rk2.hip
int ffm_panel_launch_rk3(const ffm_gemm_args& a, int cfg, hipStream_t s);      // gemm_panel_rk3.hip

int ffm_panel_launch_rk(const ffm_gemm_args& a, int cfg, hipStream_t s) {
    if (!a.rk || ((uintptr_t)a.rk & 15) || !a.S || !a.lw || a.rank <= 0 || a.rank > 16) return FFM_EINVAL;
    if ((a.flags & FFM_EPI_LGRAD) && (!a.lg_v || ((uintptr_t)a.lg_v & 15) || !a.lg_part_c || !a.lg_part_a || a.rank % 4 || a.gelu_deriv))
        return FFM_EINVAL;
    switch (cfg >= 0 && cfg < FFM_PANEL_NCFG ? FFM_PANEL_CFGS[cfg].unit : 0) {
        case 1: return ffm_panel::launch_unit<1>(a, cfg, s);
        case 2: return ffm_panel_launch_rk2(a, cfg, s);
        case 3: return ffm_panel_launch_rk3(a, cfg, s);
    }
    return FFM_EINVAL;      // (a plain row, or no row)
}
