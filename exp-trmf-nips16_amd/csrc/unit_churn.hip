// unit_churn.hip -- csr_churn_count_kernel, csr_churn_kernel, csc_gather_kernel, dense_churn_kernel and row_gather_kernel: series
// churn behind trmf_session_change_series (kernel_units.hpp: one translation unit per kernel family).  None of them is a template;
// the cold-start fit launches unit_adapt.hip's kernels.
#define TRMF_UNIT 15
#include "kernel_units.hpp"
