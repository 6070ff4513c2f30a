// pk_form.h -- which cell body the packed scorer sw128_pk_kernel runs for a parameter set (sw_kernels.hip PkVariant), as one
// inline rule without a device: make_config (swmi_api.cpp) launches by it, swmi_pk_cell_form (pk_form_kernels.hip,
// include/swmi_pk_form.h) reports it.  tests/pk_edges.py, tests/pk_flag_form.py and tests/pk_product_form.py restate it.
#pragma once
#include <cstdint>

#include "pk_product_consts_gen.inc"

namespace swmi {

// The product form's multipliers and the largest rescaled H they were verified for (gen_pk_product_consts.py)
constexpr uint16_t kPkProductRowMul[4] = SWMI_PK_PRODUCT_ROW_MUL;
constexpr uint16_t kPkProductColMul[4] = SWMI_PK_PRODUCT_COL_MUL;
constexpr int kPkProductBound = SWMI_PK_PRODUCT_BOUND;

struct PkCellForm {
    int variant;        // 0 = no bias needed, 1 = biased, 2 = vertical-offset form
    int add;            // the kernel's row bytes hold s + add (flag form: flag bytes instead, see flag_unit)
    int bias;           // variant 1: Q = -(min s + gap)
    int flag_unit;      // variant 2 only, 0 = off: m + gap of the FLAG FORM -- q0's cell on values rescaled by 255 / (m + gap);
                        // the row bytes are then 0x00 (score = m) or 0x80 (score <= -2 gap)
    int flag_gap;       // ... and the rescaled gap, 255 gap / (m + gap)
    bool product;       // flag form only: its PRODUCT FORM -- lookup and diagonal add of a row are one v_pk_mad_i16
};

//   0  every s + gap >= 0: nothing to bias
//   2  every s + 2 gap in [0, 255] and the largest value of the vertical-offset form, 128 max(s) + gap * 34 + 256,
//      stays a finite half-precision pattern (< 0x7C00): rows carry s + 2 gap
//   1  anything else: values shifted by Q = -(min s + gap)
// The flag form of 2: a score s <= -2 gap never decides a cell, so when every entry is either such a score or one
// common value m, the recurrence rescaled by 255 / (m + gap) needs one bit per entry.  It applies when
//   * the rule above gives 2,
//   * every entry is either m, with m + gap > 0, or <= -2 gap,
//   * (m + gap) divides 255 gap: the rescaled gap is an integer (and with it every rescaled H),
//   * 255 (128 m + gap) / (m + gap) + 255 < 0x7C00: the largest rescaled value, 128 matches + gap + one more folded score.
// The product form of the flag form: the diagonal term is  a[row base] * b[column base] + H(i-1,j-1)  modulo 2^16,
// which is H + 255 where the bases agree and a finite negative half where they differ.  It applies when
//   * the flag form applies,
//   * the enabled entries are exactly the four diagonal ones (plain match / mismatch scoring),
//   * the largest rescaled H, 255 * 128 m / (m + gap), is at most kPkProductBound.
inline PkCellForm pk_cell_form(const int8_t *sm, int gap)
{
    PkCellForm f = {0, gap, 0, 0, 0, false};
    int lowest = 255, highest = -255;
    for (int k = 0; k < 16; ++k) {
        lowest = int(sm[k]) < lowest ? int(sm[k]) : lowest;
        highest = int(sm[k]) > highest ? int(sm[k]) : highest;
    }
    if (lowest + gap >= 0) return f;
    if (!(lowest + 2 * gap >= 0 && highest + 2 * gap <= 255 && 128 * (highest > 0 ? highest : 0) + 34 * gap + 256 < 0x7C00)) {
        f.variant = 1;
        f.bias = -(lowest + gap);
        f.add = gap + f.bias;
        return f;
    }
    f.variant = 2;
    f.add = 2 * gap;
    bool have = false, one_value = true;
    int m = 0;
    for (int k = 0; k < 16; ++k) {
        const int s = int(sm[k]);
        if (s <= -2 * gap) continue;
        if (have && s != m) one_value = false;
        have = true;
        m = s;
    }
    const int unit = m + gap;
    if (have && one_value && unit > 0 && (255 * gap) % unit == 0 &&
        255 * (128 * m + gap) + 255 * unit < 0x7C00 * unit) {       // (the bound of the comment above, times m + gap > 0)
        f.flag_unit = unit;
        f.flag_gap = 255 * gap / unit;
        bool diagonal = true;
        for (int k = 0; k < 16; ++k) diagonal = diagonal && (int(sm[k]) > -2 * gap) == (k / 4 == k % 4);
        f.product = diagonal && 255 * 128 * m <= kPkProductBound * unit;
    }
    return f;
}

}  // namespace swmi
