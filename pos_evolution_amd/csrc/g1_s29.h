// g1_s29.h -- the XYZZ point formulas of g1_lazy.inc over the S29 field form (fp381_s29.h).  The accumulation's form in
// rounds 4-6; no kernel of the library computes points in it now (g1_s30.h), the tools that compare field forms
// (tools/fpbench_lazy.hip, tools/icbench.hip) and tests/test_host_fp29.py do.
//
// The form's bookkeeping: products come out in (-eps, p + eps) with balanced limbs (|limb| <= 2^28); a difference of two such
// values, or of two table rows (canonical limbs in [0, 2^29)), goes into the next product as it is (|limb| <= 2^29 + small).
// X3 = RR - PPP - 2 Q (|limb| <= 2^30 before the pass) and Y3 take one carry pass each and then hold |limb| <= 2^28 + 4.
// Two carry passes, six limb-wise subtractions, eight products and two squarings per mixed add: 3 738 multiply-adds.
#pragma once
#include "fp381_s29.h"  // the form's own part; the field text both forms share is fp381_lazy.inc

namespace posevo {

// a difference that feeds a product: as it is
PE_HD void fq_sub_operand(fq& r, const fq& a, const fq& b) { fq_sub(r, a, b); }
// a table row as the accumulator: one carry pass makes balanced digits of its canonical limbs (signed x signed multiplies)
PE_HD void fq_first_operand(fq& r, const fq& a) { fq_norm(r, a); }

#include "g1_lazy.inc"

}  // namespace posevo
