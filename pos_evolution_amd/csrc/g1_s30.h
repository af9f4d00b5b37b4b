// g1_s30.h -- the XYZZ point formulas of g1_lazy.inc over the S30 field form (fp381_s30.h): what k_g1_accumulate and
// k_g1_tree compute with (g1_kernels.hip); tests/test_host_fp30.py runs the same text on the CPU.
//
// The form's bookkeeping: a product accepts balanced digits only (|limb| <= 2^29 + 16), so every difference that feeds a
// product takes a carry pass: a mixed add normalises P = U2 - X1, R = S2 - Y1, X3 = RR - PPP - 2 Q, Q - X3 and Y3 (five
// passes, S29: two) around eight products and two squarings -- 3 224 multiply-adds instead of 3 738.  Registry rows are
// stored as balanced digits and are product operands as they are.
#pragma once
#include "fp381_s30.h"  // the form's own part; the field text both forms share is fp381_lazy.inc

namespace posevo {
namespace s30 {

// a difference that feeds a product: through one carry pass (|limb| up to 2^30 + 4 before it)
PE_HD void fq_sub_operand(fq& r, const fq& a, const fq& b) { fq_sub_norm(r, a, b); }
// a table row as the accumulator: its balanced digits as they are
PE_HD void fq_first_operand(fq& r, const fq& a) { r = a; }

#include "g1_lazy.inc"

}  // namespace s30
}  // namespace posevo
