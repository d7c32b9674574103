// k_liftover_brk.hip -- the break-paf build of the per-record clip kernel (rb_stream.h, BRK; launched by rb_launch_liftover_stream,
// k_liftover.hip).  A translation unit of its own because of its registers: it captures no boundaries (its pieces appear while the
// record streams), so it fits below a ring at v80..v95 and runs five waves per SIMD, which the liftover build no longer does.
#include "rb_lift.h"
#include "rb_launch.h"
#define RB_RING_BASE 80
#define RB_RING_TOP_N 95
#define RB_SPILL_ROOM 0
#define RB_WPE 5, 6
#include "rb_stream.h"

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RB_WPE), amdgpu_num_vgpr(RB_RING_BASE - RB_SPILL_ROOM))) void rb_k_liftover_stream_brk(rb_lift_params p_) {
    (void)p_; // (read through the kernel-argument segment, see the top of rb_stream_record)
    rb_stream_record<true, false>();
}
extern "C" hipError_t rb_launch_liftover_stream_brk(const rb_lift_params *p, unsigned blocks, hipStream_t stream) {
    hipLaunchKernelGGL(rb_k_liftover_stream_brk, dim3(blocks), dim3(256), 0, stream, *p);
    return hipGetLastError();
}
