// k_liftover_list.hip -- the per-record clip kernel (rb_stream.h, k_liftover.hip) over a LIST of records: the records of the tiles the tile
// kernel (k_tile.hip) handed back.  Workgroups that stay and take entry after entry.  A translation unit of its own because of its registers:
// the loop around the record's body makes the compiler park spilled scalar registers in two more vector registers than the plain
// kernels need, and it places them right behind its own allocation -- where the plain kernels kept their load ring at the time (v80..v95,
// tools/check_ring.py found them at v80 v81).  Here the ring sits at v88..v103 and the compiler is held to 84 registers: four waves
// per SIMD, on a path that sees the odd record.  (The plain kernels have their ring there too since the liftover build captures its
// boundaries; this form does not capture -- rb_stream.h, CAP -- because with the capture its build reaches v90.)
#include "rb_lift.h"
#include "rb_launch.h"
#define RB_RING_BASE 88
#define RB_RING_TOP_N 103
#define RB_SPILL_ROOM 4
#define RB_WPE 4, 5
#include "rb_stream.h"

#define RB_LIST_BLOCKS 2560u // workgroups of the list form (twice what the chip holds at five per CU: entries differ in length)
// (the loop's state is ONE vector register -- the entry index, kept opaque --: everything else is read again from the kernel-argument
//  segment per entry.  Scalar registers carried around the record's body are spilled, and this build's spills reached into the ring)
#define RB_STREAM_LIST_KERNEL(NAME, BRK)                                                                                          \
    __global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RB_WPE), amdgpu_num_vgpr(RB_RING_BASE - RB_SPILL_ROOM))) void NAME(rb_lift_params p_) { \
        (void)p_;                                                                                                                 \
        const rb_kparams kp_ = (rb_kparams)__builtin_amdgcn_kernarg_segment_ptr();                                                \
        uint32_t i_v = blockIdx.x * 4u + (threadIdx.x >> 6);                                                                      \
        for (;;) {                                                                                                                \
            asm volatile("" : "+v"(i_v));                                                                                         \
            const rb_kparams kl_ = rb_kp_here(kp_);                                                                               \
            const uint32_t i_ = rb_first(i_v);                                                                                    \
            if ((unsigned long long)i_ >= *kl_->fb_count) break;                                                                  \
            const uint64_t w_ = rb_first(kl_->slot_of[rb_first(kl_->fb_list[i_])]);                                               \
            rb_stream_record<BRK, false, true>(w_);                                                                               \
            i_v += RB_LIST_BLOCKS * 4u;                                                                                           \
        }                                                                                                                         \
    }
RB_STREAM_LIST_KERNEL(rb_k_liftover_stream_list, false)
RB_STREAM_LIST_KERNEL(rb_k_liftover_stream_brk_list, true)
extern "C" hipError_t rb_launch_liftover_stream_list(const rb_lift_params *p, hipStream_t stream) {
    if (p->n_rec == 0 || p->n_tiles == 0) return hipSuccess;
    if (p->brk_mode) hipLaunchKernelGGL(rb_k_liftover_stream_brk_list, dim3(RB_LIST_BLOCKS), dim3(256), 0, stream, *p);
    else hipLaunchKernelGGL(rb_k_liftover_stream_list, dim3(RB_LIST_BLOCKS), dim3(256), 0, stream, *p);
    return hipGetLastError();
}
