// The library's A/B switches: one table, read from the environment once per process (at the first ffm_sw() call of any
// translation unit, main object or IEEE-half twin alike), read-only afterwards, readable from outside through ffm_switch
// (include/ffm_hip.h).  What a switch decides, and what was measured with it, is written where the decision is made;
// this file says only how each variable is parsed.  The engines' own switches: fairfedmed_amd/engine.py (Switches).
#pragma once

// defaults a diagnostic build may override (-D on switches.hip)
#ifndef FFM_PANEL_MASK_DEFAULT
#define FFM_PANEL_MASK_DEFAULT ((1 << 7) | (1 << 8) | (1 << 10))      // gemm_panel.hip: what the bits are
#endif
#ifndef FFM_SKINNY_CAP_DEFAULT
#define FFM_SKINNY_CAP_DEFAULT 0
#endif
#ifndef FFM_SKINNY_NT_DEFAULT
#define FFM_SKINNY_NT_DEFAULT 2
#endif
#ifndef FFM_SKINNY_MINB_DEFAULT
#define FFM_SKINNY_MINB_DEFAULT 1
#endif

// X(field, variable, rule, default, meaning).  An unset variable gives `default`; a set one gives rule(its string):
//   sw_o0   1 for a first character '0' or 'o', but 0 for "on"       sw_int   atoi, nothing validated
//   sw_o    1 when the first character is 'o', else 0                 sw_oint  -1 when the first character is 'o', else atoi
//   sw_not0 0 when the first character is '0', else 1                 sw_vgen  "v1" / "v2" / "v3" -> 1 / 2 / 3, else 0
//   sw_4    4 when the first character is '4', else 2
// A default may name a field of an earlier row (`sw.`: the table being filled).
#define FFM_SWITCH_TABLE(X)                                                                                                      \
    X(panel_off,         "FFM_PANEL",             sw_o0,   0,                       "off: never a panel tile, always the 128x128 kernel") \
    X(panel_mask,        "FFM_PANEL_MASK",        sw_int,  FFM_PANEL_MASK_DEFAULT,  "bit <row> enables a masked row of the panel table") \
    X(skinny_off,        "FFM_SKINNY",            sw_o,    0,                       "off: skinny products on the 128x128 kernel (split-operand ones excepted)") \
    X(skinny_splitk,     "FFM_SKINNY_SPLITK",     sw_int,  2048,                    "widest N of a skinny product that is split over K; 0: none") \
    X(skinny_splitk_min, "FFM_SKINNY_SPLITK_MIN", sw_int,  4,                       "fewest 128-wide K slices of a split product") \
    X(skinny_cap,        "FFM_SKINNY_CAP",        sw_int,  FFM_SKINNY_CAP_DEFAULT,  "most blocks of a skinny launch; 0: one per tile") \
    X(skinny_nt,         "FFM_SKINNY_NT",         sw_int,  FFM_SKINNY_NT_DEFAULT,   "column tiles per block of the split-operand product: 1 | 2 | 4") \
    X(skinny_nt_narrow,  "FFM_SKINNY_NT_NARROW",  sw_int,  sw.skinny_nt,            "the same for N <= 512") \
    X(skinny_minb,       "FFM_SKINNY_MINB",       sw_int,  FFM_SKINNY_MINB_DEFAULT, "fewest blocks that tiling may leave such a launch") \
    X(gemm_deep,         "FFM_GEMM_DEEP",         sw_not0, 1,                       "0: no four-stage ring in the 128x128 GEMM") \
    X(conv_deep,         "FFM_CONV_DEEP",         sw_not0, 1,                       "0: the two-buffer split-K plan of the 3x3 convolution") \
    X(conv_narrow_max,   "FFM_CONV_NARROW",       sw_oint, 0,                       "off (-1): no 128xN convolution tiles; t: also below t 128x128 tiles") \
    X(attn_gen,          "FFM_ATTN",              sw_vgen, 0,                       "v1 | v2 | v3: the newest attention generation allowed; 0: all (= v3)") \
    X(attn_parts,        "FFM_ATTN_PARTS",        sw_4,    2,                       "4: second-generation attention on quarter heads") \
    X(attn3_map,         "FFM_ATTN3_MAP",         sw_not0, 1,                       "0: third-generation attention spreads an image's heads over the XCDs") \
    X(bn_fold_rows,      "FFM_BN_FOLD_ROWS",      sw_int,  32768,                   "most rows of a BatchNorm that runs without the finalize launch") \
    X(bn_rpt,            "FFM_BN_RPT",            sw_int,  2,                       "rows per thread of the BatchNorm apply kernels")

struct ffm_switches {
#define X(field, var, rule, dflt, doc) int field;
    FFM_SWITCH_TABLE(X)
#undef X
};

const ffm_switches& ffm_sw();
