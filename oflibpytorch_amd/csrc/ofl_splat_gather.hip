// ofl_splat_gather.hip -- the gather splat's round-6 kernel (splat_gather2_kernel: in-order sums on a register / LDS diet, three
// 512-thread blocks per CU) as a translation unit of its own: ofl_kernels.hip holds the kernel and its helpers, this file instantiates
// it -- for fp32 operands, for fp16-stored flows and for an fp32 flow with fp16 / bf16 data and results (ofl_splat_sum_x16) -- so that
// its instantiations compile in parallel with the rest of the library.  Exports one function to the other translation units:
// ofl_splat_launch_gather_diet.
#define OFL_SPLAT_TU 1
#include "ofl_kernels.hip"
