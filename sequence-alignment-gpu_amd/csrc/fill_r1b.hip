// Fill kernels for R = 1 chains of DNA-sized alphabets with three-row bands (192-row score strips
// feeding strip groups of three, sa_fill.hip process_band3): a code object of its own, so the two-row
// kernels of fill_r1.hip are unchanged.
#define SA_FILL_R 1
#define SA_FILL_TU_BAND3 1
#include "sa_fill.hip"
