// Internal interface between gemm.hip (dispatcher, 128x128 kernel) and gemm_panel*.hip (panel kernel).
//
// Everything that says "panel kernel (tile configuration c, epilogue F) exists" is in this file, once: the geometry and the
// capabilities of a tile are its row of FFM_PANEL_CFGS, the epilogue words are the two lists FFM_PANEL_EPI_*, and
// ffm_panel_has(c, F) combines them.  The selector asks it (gemm_panel.hip).  The launch code is generated from the same
// rows (gemm_panel_impl.h): the unit a row names in `unit` instantiates launch_unit<unit>, which holds launch_row<c> for
// every built row with that number and, through ffm_panel_has, every epilogue of the row.  So a pair the selector can
// return is instantiated, provided `unit` is a unit that exists: the static_assert under the table holds it to that.
// To add or retire a tile: edit its row.  To enable a masked one by default: its bit in FFM_PANEL_MASK_DEFAULT
// (gemm_panel.hip).  Nothing else.
#pragma once
#include "common.h"

// Panel-kernel tile configurations: block tile (16*MF) x (16*PW*NF), PW waves side by side along N, 16*NF columns each.
// PW = 4: one wave per SIMD (up to 312 accumulator registers per wave); PW = 8: two waves per SIMD (<= 256 registers).
// With PW = 4, MF is chosen so that the A-ring pieces, 2*MF (+2 for the rank rows under FFM_EPI_RANKOP), split evenly
// over the waves; with PW = 8 the waves that run out of pieces repeat one (gemm_panel_impl.h, PanelGeom).
struct ffm_panel_cfg {
    int mf, nf;
    bool rankop;     // instantiated for the FFM_EPI_RANKOP epilogues (true) or for the plain ones (false)
    int per_cu;      // blocks that share a CU (registers + LDS): a round is 256 * per_cu blocks
    int pw;          // waves per block
    int ks;          // 1: the 8 waves are 4 column slabs x 2 K halves (gemm_panel_impl.h, KS) - the tile is 64*nf wide
    bool built;      // false: measured, lost, not instantiated any more (the row stays: indices and mask bits do not move)
    bool masked;     // selected only with bit <index> of FFM_PANEL_MASK set (switches.h: FFM_PANEL_MASK_DEFAULT)
    bool lgrad;      // has the FFM_EPI_LGRAD epilogues
    bool lnb_apply;  // has the FFM_EPI_LNB_APPLY epilogue
    int min_k;       // not selected for a shorter K (0: no limit of its own)
    int unit;        // the translation unit that instantiates the row: 0 gemm_panel.hip (plain), 1 / 2 / 3 gemm_panel_rk /
                     // _rk2 / _rk3.hip (FairLoRA: split for compile time, one unit took 6.5 minutes)
    bool lora_plain = false;  // has the FairLoRA word without GELU or residual (the adapted qkv forward, N = 3 x width)
};
constexpr int FFM_PANEL_NCFG = 13;
constexpr ffm_panel_cfg FFM_PANEL_CFGS[FFM_PANEL_NCFG] = {
    // one wave per SIMD (round 2)
    {13, 6, true, 1, 4, 0, true, false, false, false, 0, 1},    //  0: 208x384 FairLoRA
    // 1: measured (tools/bench_panel.py): with a short K the 256-wide tile does not pay for the un-overlapped prologue /
    // store burst of a single round (qkv, K = 768: 34.6 us against 32.5 us)
    {16, 4, false, 1, 4, 0, true, false, false, false, 1536, 0}, //  1: 256x256 plain
    {10, 2, false, 1, 4, 0, true, false, false, true, 0, 0},    //  2: 160x128 plain
    {11, 2, true, 1, 4, 0, true, false, false, false, 0, 1},    //  3: 176x128 FairLoRA
    {8, 4, false, 2, 4, 0, true, false, false, false, 0, 0},    //  4: 128x256 plain, two blocks per CU
    // two waves per SIMD: the same tiles as 3, 2 (5, 6: eight column slabs, no gain, twice the LDS fragment reads) and 0
    {11, 1, true, 1, 8, 0, false, true, false, false, 0, 1},    //  5: 176x128 FairLoRA
    {10, 1, false, 1, 8, 0, false, true, false, false, 0, 0},   //  6: 160x128 plain
    // (7 also serves the adapted in-projection with ln_1 folded in: 186 blocks at 6304 x 2304, where the 128-column FairLoRA
    // tiles need 720.  The same product WITHOUT the fold, FFM_EPI_BIAS | FFM_EPI_LORA, measured 40.0 us on this tile against
    // 39.6 us on the 128x128 kernel (tools/bench_panel.py --attn) and has no panel word)
    {13, 3, true, 1, 8, 0, true, true, true, false, 0, 3, true}, //  7: 208x384 FairLoRA
    // 8: the 160-row FairLoRA tile for N = 768 (240 blocks at 6304 rows where the 176-row tile launches 216); 9 / 10:
    // 240 x 256 for qkv (243 blocks), one and two waves per SIMD
    {10, 2, true, 1, 4, 0, true, true, false, true, 0, 2},      //  8: 160x128 FairLoRA
    {15, 4, false, 1, 4, 0, false, true, false, false, 0, 0},   //  9: 240x256 plain
    {15, 2, false, 1, 8, 0, true, true, false, false, 0, 0},    // 10: 240x256 plain
    // 11 / 12: the 160x128 tiles with 8 waves as 4 column slabs x 2 K halves (K % 256 == 0)
    {10, 2, true, 1, 8, 1, true, true, false, false, 0, 2},     // 11: 160x128 FairLoRA
    {10, 2, false, 1, 8, 1, true, true, false, false, 0, 0}};   // 12: 160x128 plain

constexpr bool ffm_panel_units_exist() {
    for (const ffm_panel_cfg& c : FFM_PANEL_CFGS)
        if (c.built && (c.rankop ? c.unit < 1 || c.unit > 3 : c.unit != 0)) return false;
    return true;
}
static_assert(ffm_panel_units_exist(), "a built row names the unit that instantiates it: 0 if plain, 1..3 if FairLoRA");

struct ffm_panel_tile {
    int bm, bn, waves;      // rows, columns, waves per CU
};
constexpr ffm_panel_tile ffm_panel_tile_of(const ffm_panel_cfg& c) {
    return {16 * c.mf, 16 * (c.ks ? c.pw / 2 : c.pw) * c.nf, c.pw * c.per_cu};
}

// The epilogue words with a panel kernel, per family, without FFM_EPI_RANKOP (the row says which family it is built for).
// FFM_EPI_GELU_ONLY is not listed: it exists exactly where the word with FFM_EPI_GELU exists.
#define FFM_PANEL_EPI_PLAIN(X)                                                                                          \
    X(0)                                                                                                                \
    X(FFM_EPI_BIAS)                                                                                                     \
    X(FFM_EPI_BIAS | FFM_EPI_RESIDUAL)                                                                                  \
    X(FFM_EPI_BIAS | FFM_EPI_RESIDUAL | FFM_EPI_ROWSTATS) /* out-proj forward leaving row sums for ln_2 */              \
    X(FFM_EPI_BIAS | FFM_EPI_LNIN)                        /* qkv forward with ln_1 folded in */                         \
    X(FFM_EPI_LNB_APPLY)                                  /* dX of qkv applying ln_1's backward */
#define FFM_PANEL_EPI_RK(X)                                                                                             \
    X(FFM_EPI_BIAS | FFM_EPI_LORA | FFM_EPI_LNIN)       /* adapted qkv forward with ln_1 folded in (rows with lora_plain) */ \
    X(FFM_EPI_BIAS | FFM_EPI_LORA | FFM_EPI_GELU)                           /* c_fc forward */                          \
    X(FFM_EPI_BIAS | FFM_EPI_LORA | FFM_EPI_GELU | FFM_EPI_LNIN)            /* ... with ln_2 folded in */               \
    X(FFM_EPI_BIAS | FFM_EPI_LORA | FFM_EPI_RESIDUAL)                       /* c_proj forward */                        \
    X(FFM_EPI_BIAS | FFM_EPI_LORA | FFM_EPI_RESIDUAL | FFM_EPI_ROWSTATS)    /* ... leaving row sums for ln_1 */         \
    X(FFM_EPI_LORA | FFM_EPI_LORA_KR | FFM_EPI_DGELU)                       /* dX of c_proj */                          \
    X(FFM_EPI_LORA | FFM_EPI_LORA_KR | FFM_EPI_DGELU | FFM_EPI_LGRAD)       /* ... with the two gradient partial products */ \
    X(FFM_EPI_LORA | FFM_EPI_LORA_KR | FFM_EPI_DGELU | FFM_EPI_LGRAD | FFM_EPI_LNB_STAT) /* ... and ln_2's backward row sums */ \
    X(FFM_EPI_LORA | FFM_EPI_LORA_KR)                                       /* dX of c_fc */                            \
    X(FFM_EPI_LORA | FFM_EPI_LORA_KR | FFM_EPI_LNB_APPLY)                   /* ... applying ln_2's backward */

// Does the panel kernel (configuration c, epilogue word f without FFM_EPI_RANKOP) exist?
constexpr bool ffm_panel_has(int c, int f) {
    const ffm_panel_cfg& cf = FFM_PANEL_CFGS[c];
    if (f & FFM_EPI_GELU) f &= ~FFM_EPI_GELU_ONLY;
    bool listed = false;
#define FFM_PANEL_WORD(W) listed = listed || f == (W);
    if (cf.rankop) {
        FFM_PANEL_EPI_RK(FFM_PANEL_WORD)
    } else {
        FFM_PANEL_EPI_PLAIN(FFM_PANEL_WORD)
    }
#undef FFM_PANEL_WORD
    if (!cf.built || !listed) return false;
    if ((f & FFM_EPI_ROWSTATS) && ((2 * cf.nf) & (2 * cf.nf - 1))) return false;      // row sums: power-of-two lanes per row
    if ((f & FFM_EPI_LGRAD) && !cf.lgrad) return false;
    if ((f & FFM_EPI_LNB_APPLY) && !cf.lnb_apply) return false;
    if (cf.rankop && !(f & (FFM_EPI_GELU | FFM_EPI_RESIDUAL | FFM_EPI_LORA_KR)) && !cf.lora_plain) return false;
    return true;
}

// -1: use the 128x128 kernel; otherwise the index into FFM_PANEL_CFGS
int ffm_panel_select(int M, int N, int K, int flags, int rank, int dtype, bool packed);
int ffm_panel_launch(const ffm_gemm_args& a, int cfg, hipStream_t s);
int ffm_panel_launch_rk(const ffm_gemm_args& a, int cfg, hipStream_t s);      // gemm_panel_rk.hip

// gemm_skinny.hip: M <= 64 rows (text tower), bf16 / f32, plain epilogues
bool ffm_skinny_ok(const ffm_gemm_args& a, int dtype);
int ffm_skinny_launch(const ffm_gemm_args& a, int dtype, hipStream_t s);
