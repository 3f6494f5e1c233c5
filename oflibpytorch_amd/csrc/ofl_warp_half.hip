// ofl_warp_half.hip -- the staged backward-warp kernels once more, for planes STORED in fp16 / bf16 (ofl_warp_bwd_x16: Flow.apply /
// apply_flow 't' of a feature tensor held in half precision).  The kernels of ofl_kernels.hip are templates on the source and
// destination element type; this translation unit instantiates them for half_t and bf16_t (up-conversion at the load -- exact --,
// the same fp32 arithmetic, one round-to-nearest-even at the store) on 64 x 16 tiles, as ofl_warp_wide.hip does for fp32, and holds
// their launcher (the OFL_X16_TU section of ofl_kernels.hip).  The same section holds the flow gradient of that warp
// (ofl_warp_bwd_grad_x16: the GRAD instantiations on 16-bit taps and a 16-bit upstream gradient, a one-pixel-per-lane kernel from 4
// planes on).  Compiled side by side with the other units (_build.py); the fp32 units do not see these instantiations.
#define OFL_X16_TU 1
#define OFL_LDS_NT 256
#define OFL_LDS_TWQ 16
#define OFL_LDS_BYTES 53248
#include "ofl_kernels.hip"
