// mhs_values_mixed.hip -- the forward kernels of the mixed values plans (FP32 values, FP64 sums:
// mhs_values_plan_create_accum), a translation unit of their own: the templates of mhs_values.hip instantiated at
// <float, W, PlusTimes, double>, W = 1, 2, 4, with init_values_mixed_attributes and issue_values_mixed (declared in
// mhs_valwalk.hpp).  Kept apart so that the code object of mhs_values.hip holds what it held before.
#define MHS_VALUES_MIXED_TU 1
#include "mhs_values.hip"
