// print_fold.h — the value of one cell of a PRINT search, defined once for the kernels of print_cascade.hip.  A print's view has its minutiae template in slot 0 and its
// texture template in slot 3; with the query's two weights — the host has written a zero where the term is not active (the print does not hold the template, or the
// caller's weight is zero), so "active" is w != 0.0f — the cell of a column that is neither empty nor removed is
//   -1.0f                                    where nothing is active
//   (float)acc                               otherwise: double acc = +0.0; minutiae active: acc = acc + (double)w_m * (double)v_m; then texture active:
//                                            acc = acc + (double)w_t * (double)v_t
// which is template_fold.hip's k_fold_templates for one pseudo-query of that view and its k_fold_print_pairs, bit for bit: the product of two fp32 values is exact in
// fp64, both products are formed whether used or not and left out by a select, and the first add to +0.0 is made (it turns a product of -0.0 into +0.0).
#pragma once
#include <hip/hip_runtime.h>

namespace afis {

__device__ __forceinline__ float fold_print_cell(float w_m, float v_m, float w_t, float v_t)
{
    const bool am = w_m != 0.0f, at = w_t != 0.0f;
    const double pm = (double)w_m * (double)v_m, pt = (double)w_t * (double)v_t;
    double acc = 0.0;
    acc = am ? acc + pm : acc;
    acc = at ? acc + pt : acc;
    return am || at ? (float)acc : -1.0f;
}

}  // namespace afis
