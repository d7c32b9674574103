// rb_stream.h -- the per-record streaming clip kernel's body, rb_stream_record<BRK, DIAG, LIST> (see the head of k_liftover.hip for
// what it does), with the load ring it keeps in vector registers the compiler cannot see.  Included once by each of its three users,
// which differ in where the ring sits and define, in front of the #include:
//   RB_RING_BASE    first register of the ring; the compiler is held to the registers below it (amdgpu_num_vgpr)
//   RB_RING_TOP_N   last register of the ring (RB_RING_BASE + 15)
//   RB_SPILL_ROOM   registers between the compiler's allocation and the ring, for the VGPRs it parks spilled scalar registers in
//   RB_WPE          waves per SIMD the register budget is cut for (amdgpu_waves_per_eu: "min, max")
// k_liftover.hip: 88, 103, 4, (4, 5) -- the liftover kernel; k_liftover_brk.hip: 80, 95, 0, (5, 6) -- break-paf; k_liftover_list.hip:
// 88, 103, 4, (4, 5) -- the list kernels.
// (the liftover kernel had the ring at v80 and five waves per SIMD until it began to capture its boundaries in the step: with the
//  capture the compiler wants 81 registers and two more for its spilled scalars; round 4 measured four waves at +0.5 %)
// tools/check_ring.py disassembles all three and fails if the compiler names a register of the ring.
// Boundaries: a step that streams the chunk holding a clip's start or end offset leaves the chunk's 8 ops, the op in front and the
// prefixes in an LDS entry of that boundary, and the resolution behind the segment reads the entry instead of loading the group from
// the record a second time (by then out of L2: ~100 bytes fetched per boundary, a dependent trip with the ring drained).
//
// One configuration is built, the one rounds 2 - 5 arrived at (docs/history.md, profiles/r04_stream_summary.md); what lost, in a line each:
//   a lane's 8 ops as 32 contiguous bytes, where every load and store instruction touches all sixteen 128-byte lines of the step and
//     moves half of each: liftover 9.29 against 9.08 ms a step (kernel 9.08 against 8.87 ms), break-paf 8.04 against 7.75 ms, three runs
//     each in alternation (profiles/stream_flat_summary.md).  The step is flat in all three users: lane l holds the 4-op groups l and
//     l + 64 of the step, and every instruction covers 1 KiB of whole lines (the memory-mix probe prices the shapes at 7.62 and 7.19 ms);
//   half-sized flat steps of 4 ops per lane: 2 % (11.81 against 12.07 ms) for twice the wave scans and scalar bookkeeping per op, ring at v96;
//   three steps in flight instead of two (ring at v96, four waves per SIMD instead of five), segments of 12 steps: nothing;
//   non-temporal stores of the stream: 2 ms longer; non-temporal loads: 5 - 17 % slower; a touch load of a later wave's job: nothing;
//   a separate interior ("fast") step: 84 vector registers, the ring at v96, 9.81 against 9.74 ms on one box;
//   no preload of the ring in front of the window loads: nothing measurable, the preload is the shorter chain;
//   end ops patched by rewriting their 16-byte groups or whole granules: 9.5 / 10.3 / 11.6 ms for 16 / 64 / 128 bytes on one box;
//   store granules of 128 bytes instead of 64: nothing, against -0.6 % / -1.7 % (fast / slow box) for 64 bytes over none.
#pragma once
#include "rb_lift.h"
#include <type_traits>

#if !defined(RB_RING_BASE) || !defined(RB_RING_TOP_N) || !defined(RB_SPILL_ROOM) || !defined(RB_WPE)
#error "rb_stream.h: define RB_RING_BASE, RB_RING_TOP_N, RB_SPILL_ROOM and RB_WPE in front of the #include"
#endif

// diagnostics (debug_skip & 32): shader-clock time of each phase of a record, every 16th record, summed in units of 16
// cycles into counters->phase[0..4]: job + windows, stream + resolve, verdict + finalize, reservation, rows + end ops
#define RB_PHASE(i)                                                                                                  \
    if (dbg & 32) {                                                                                                  \
        const long long t_now = clock64();                                                                           \
        if (lane == 0 && (wave & 15) == 0) atomicAdd(&p.counters->phase[i], (uint32_t)((t_now - t_prev) >> 4));       \
        t_prev = t_now;                                                                                              \
    }

// A step is 512 ops: two 16-byte loads per lane, 256 ops apart (lane l: ops 4 l .. 4 l + 3 of each half of the step).
#define RB_OPL 8                                   // ops per lane and step
#define RB_GRP 2                                   // 16-byte groups per lane and step
#define RB_STEP_SHIFT 9                            // log2 of the ops of a step
#define RB_PF 2                                    // steps of stream loads in flight per wave (4 KiB)
#define RB_SMAX 10                                 // steps whose checkpoints fit in LDS at once; whole turns of the load ring
static_assert(RB_GRP * 4 == RB_OPL && (1 << RB_STEP_SHIFT) == 64 * RB_OPL && RB_CP_OPS == RB_OPL && RB_SMAX % RB_PF == 0, "the shape of a step");
// vector-memory instructions a step of the streaming loop issues, always (stores whose mask is empty are issued with an empty
// exec mask: they move nothing but they count, tools/vmcnt_probe.hip, which keeps every s_waitcnt immediate exact)
#define RB_STEP_VMEM (RB_GRP * RB_MS + RB_GRP)
#define RB_RING_WAIT ((RB_PF - 1) * RB_STEP_VMEM) // all but the youngest of them: the loads of the step being taken have landed
// the speculative stores of a step are widened to whole granules of 64 bytes (four lanes of one half), see the stores of a step
#define RB_GRAN 16

// The load ring lives in VGPRs the compiler does not know: it allocates v0 .. v(RB_RING_BASE - 1) (amdgpu_num_vgpr), the ring is
// v[RB_RING_BASE .. RB_RING_BASE + 8 RB_PF), named literally in the asm statements that load, store and copy it out.  A ring the
// compiler can see gets copied between registers where two code paths meet (phi copies) -- harmless for ordinary values, fatal
// for registers with a load in flight, which no s_waitcnt of the compiler's covers.
#define RB_STR2(x) #x
#define RB_STR(x) RB_STR2(x)
static_assert(RB_RING_TOP_N == RB_RING_BASE + 8 * RB_PF - 1, "the ring is RB_PF slots of eight registers");
#define RB_RING_TOP "v" RB_STR(RB_RING_TOP_N) // the last register of the ring: named as a clobber so that the kernel's register count covers it
// (NOT all sixteen: a register named as clobbered is one the compiler may use for its own temporaries between two asm statements --
//  tried, it did.  What keeps the compiler out of the ring is amdgpu_num_vgpr, with one gap: the VGPRs it spills scalar registers into
//  are placed behind its own allocation, and one build of this kernel had them at v78 v79 v80.  tests/test_ring_registers.py
//  and tests/test_ring_registers_brk.py disassemble every build and fail if anything outside the asm statements names a register of the ring.)
// registers OFF .. OFF + W of the ring, as the assembler reads them (it evaluates the sums)
#define RB_RREG(OFF, W) "v[" RB_STR(RB_RING_BASE) "+" #OFF ":" RB_STR(RB_RING_BASE) "+" #OFF "+" #W "]"
#define RB_RREG1(OFF) "v[" RB_STR(RB_RING_BASE) "+" #OFF "+1]" // the second register of the pair at OFF
typedef uint32_t rb_u32x4 __attribute__((ext_vector_type(4)));
// the LDS byte address of a __shared__ object, for the asm statements that write LDS from the ring
__device__ __forceinline__ uint32_t rb_lds_addr(const void *q) { return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void *)q; }
// RB_RING_CASE(ring, M): M(<the slot's registers>) for the ring slot `ring` (a compile-time constant)
#define RB_RING_CASE(RING, M)                                                                                                   \
    if constexpr ((RING) == 0) { M(0, 2, 4, 6) } else { M(8, 10, 12, 14) }
// BRK: break-paf in one walk (rb_lift.h, brk_max): the windows of a record are not given, they are the stretches between the indels
// longer than brk_max, found while the record streams; 32 pieces a pass.  The liftover build has none of that code.
// DIAG: the diagnostics build of the same kernel (bench.py --debug-skip: phases switched off, phase timers, clock stamps); the product
// launches DIAG = false, in which no stamp executes and no debug bit is looked at.
// LIST_WAVE: the schedule slot comes from the caller (rb_k_liftover_stream_list: the records the tile kernel handed back, k_tile.hip)
template <bool BRK, bool DIAG, bool LIST = false>
__device__ __forceinline__ void rb_stream_record(const uint64_t list_wave = 0) {
    // The 408 bytes of parameters are NOT read through `p_`: the compiler loads every by-value kernel argument a kernel uses in
    // its entry block and then carries -- spills -- those hundred scalar registers through the whole record (round 2: 233 SGPR
    // spills, parked in VGPRs right under the load ring).  `p.field` below reads the field from the kernel-argument segment where
    // it is used, through a pointer the compiler cannot see through (one s_load at that place); what the streaming loop needs is
    // copied into locals in front of it.
    const rb_kparams kp = (rb_kparams)__builtin_amdgcn_kernarg_segment_ptr();
    rb_kparams kq = rb_kp_here(kp); // the pointer of the current phase (set-up / after the stream of a pass): loads through it stay inside the phase
#define p (*kq)
    // diagnostics (bench.py --debug-skip: phases of the kernel switched off, phase timers, clock stamps) only in the DIAG
    // instantiation: every tested bit is a wave-uniform boolean, i.e. two scalar registers held through the whole record
    const int dbg = DIAG ? p.debug_skip : 0;
    // checkpoints: exclusive (R,Q,U) prefixes every CPO ops, SoA so that R can be binary-searched.  The liftover build resolves from
    // what the step captured (cap_all below) and searches the checkpoints only for the boundaries the capture did not take: it keeps one
    // per 16 ops (every fourth lane of a half leaves one; the fallback loads 16 ops and picks the half, rb_load_group_wide), which makes
    // the room for the capture table.  The break build and the list form capture nothing and keep one per 8 ops (every second lane).
    // (the list form, like break-paf, captures nothing: with the capture its build reaches v87 and parks its spilled scalars in v88 v89,
    //  the first registers of its ring, which tests/test_ring_registers.py holds at v88..v103)
    constexpr bool CAP = !BRK && !LIST;
    constexpr uint32_t CPO = CAP ? 2u * RB_CP_OPS : (uint32_t)RB_CP_OPS, CPS = (64u * RB_OPL) / CPO; // ops per checkpoint, checkpoints per step
    __shared__ uint32_t cp_all[4][3][RB_SMAX * CPS];
    __shared__ uint32_t wx_all[4][RB_HMAX + 1]; // window indices of one pass over a window list that is not sorted
    // the capture table: entry b of a wave belongs to boundary b of the pass (lane b resolves it: b < 32 the start of clip b, else the
    // end of clip b - 32) and holds what the lane pair that streamed the boundary's chunk had in registers: its 8 ops (aligned to 8: the
    // groups of lanes l & ~1 and l | 1 of one half), {the op in front of them, the exclusive R, Q, U prefixes at the first of them} -- 48
    // bytes --, and in cap_t the chunk's number in the segment, in units of 8 ops
    __shared__ uint4 cap_all[CAP ? 4 : 1][CAP ? 64 * 3 : 1];
    __shared__ uint32_t cap_t[CAP ? 4 : 1][CAP ? 64 : 1];
    // LDS per block: liftover 15,360 + 528 + 12,288 + 1,024 = 29,200 bytes, break-paf and the list form 30,720 + 528 + 16 + 4 = 31,268
    static_assert(sizeof(cp_all) + sizeof(wx_all) + sizeof(cap_all) + sizeof(cap_t) == (CAP ? 29200u : 31268u), "LDS of a block");
    { // a block is four waves, one per SIMD: the waves per SIMD the build is cut for (RB_WPE, the lower figure) are its blocks per CU
        constexpr uint32_t wpe_[2] = {RB_WPE};
        static_assert(wpe_[0] * (sizeof(cp_all) + sizeof(wx_all) + sizeof(cap_all) + sizeof(cap_t)) <= 163840u, "LDS of the blocks of a CU");
    }
    const uint32_t wib = rb_first(threadIdx.x >> 6); // wave in block (told to the compiler as the wave-uniform value it is)
    uint64_t wave;
    if constexpr (LIST) {
        wave = list_wave;
    } else {
        wave = (uint64_t)p.wave0 + (uint64_t)blockIdx.x * 4u + wib;
        if (wave >= p.wave_end) return;
    }
    const int lane = rb_lane();
    long long t_prev = (dbg & 32) ? clock64() : 0;
    uint32_t *cpR = cp_all[wib][0], *cpQ = cp_all[wib][1], *cpU = cp_all[wib][2];
    const rb_job jb_ = p.jobs[wave]; // (uniform address: one 64-byte request)
    const uint32_t jflags = rb_first(jb_.flags);
    if (jflags & RB_JOB_ROWS_OVERFLOW) { // rows do not fit: flag and leave (host retries with more room)
        if (lane == 0) p.counters->overflow = 1;
        return;
    }
    if (!(jflags & RB_JOB_VALID)) return;
    const uint32_t r = rb_first(jb_.r);
    const rb_norm_row *nr = &p.norm[r];
    const uint64_t h0 = rb_first(jb_.h0);
    const uint64_t nh = rb_first(jb_.nh);
    const bool explicit_w = BRK || p.x_st != nullptr;
    const bool mono = BRK || (jflags & RB_JOB_MONO) != 0;
    uint64_t ws = 0, we = 0;
    if (!explicit_w && (!mono || !(jflags & RB_JOB_REGULAR))) { // the contig's window slice: only the rare paths need it
        const uint32_t cg = p.contig[r];
        ws = p.cw_off[cg];
        we = p.cw_off[cg + 1];
    }
    // BRK: this record is not the one-walk path's: on the list it goes (rb_k_break_pieces finds its pieces, the generic kernel clips them)
    // (one store here: rb_k_break_list_declined collects the marked records afterwards -- the list and its counter would be two more
    //  pointers for this kernel to carry)
    auto brk_decline = [&]() {
        if (lane == 0) p.brk_off[r] = ~1ull;
    };
    if (!(jflags & RB_JOB_REGULAR)) { // window order does not matter on the fast path: resolution is per lane
        if (p.fused && lane == 0) { // (a provisional row that cannot take the fast path: the full scan completes it)
            const unsigned long long i = atomicAdd(p.pend_count, 1ull);
            p.pend_list[i] = r;
        }
        if constexpr (BRK) {
            brk_decline();
            return;
        }
        rb_defer_record(kp, r, nr, h0, nh, explicit_w, mono, ws, we, lane);
        return;
    }
    // the record's coordinates are needed in front of the stream of a pass (the boundaries' offsets) and behind it (the rows), not in
    // between: they are read again from the job behind the stream instead of being carried -- in eight scalar registers, round 2 --
    // through it (the job is 64 bytes at an address the whole wave shares)
    // (coord_reload: the liftover build is better off with the round-2 form -- pinned to scalar registers --, the break build with
    //  the reload; what decides is where the compiler then parks its spilled scalar registers, tools/check_ring.py)
    auto sgpr64 = [](uint64_t v) -> uint64_t {
        uint32_t lo = rb_first((uint32_t)v), hi = rb_first((uint32_t)(v >> 32));
        asm volatile("" : "+s"(lo), "+s"(hi));
        return ((uint64_t)hi << 32) | lo;
    };
    constexpr bool coord_reload = BRK;
    uint64_t t_st = jb_.t_st, t_en = jb_.t_en, q_st = jb_.q_st, q_en = jb_.q_en;
    if constexpr (!coord_reload) t_st = sgpr64(t_st), t_en = sgpr64(t_en), q_st = sgpr64(q_st), q_en = sgpr64(q_en);
    const uint32_t n = rb_first(jb_.n);
    const uint64_t rec0 = rb_first64(jb_.rec0); // global index of the record's first kept op
    const uint32_t *rec_ops = p.ops + rec0;
    const uint64_t lo = rb_first(jb_.lo);
    uint64_t scan_pos = ws; // non-monotone window lists: next window of the slice to test
    // the stream starts on the 128-byte line that holds the record's first op: loads and stores of a step then cover whole lines
    const uint64_t g0 = rec0 & ~31ull, gend = rec0 + n;
    const uint32_t n_steps = (uint32_t)((gend - g0 + (1u << RB_STEP_SHIFT) - 1u) >> RB_STEP_SHIFT);
    const int32_t head = (int32_t)(rec0 - g0); // 0..31 ops of the previous record (or nothing) in front of the record in step 0
    const uint32_t *__restrict__ gbase0 = p.ops + g0;
    const uint32_t first_boff = (uint32_t)head * 4u;                          // byte offset (from g0) of the record's first op
    const uint32_t last_boff = (uint32_t)(((gend - 1u) & ~3ull) - g0) * 4u;   // ... of the last 16-byte group that holds an op of it

    // ---- where clips go.  Output copy ("slot") k of the batch mirrors the input positions: the op at coordinate c of this
    //      record (c counted from g0, the first op of the record's first 128-byte line) lives at
    //      out_ops[k * slot_stride + 32 r + g0 + c].  The 32 r keeps the lines of neighbouring records apart (they share one in
    //      the input when a record does not start on a multiple of 32).  Clip j of the record goes to slot j mod n_slots, so a step of the stream can be stored
    //      from the registers it was loaded into, with the aligned address it was loaded from: no size is needed to place a
    //      clip, hence no reservation, no atomic and no second read of the ops. ----
    const uint32_t n_slots = (uint32_t)p.n_slots;
    uint32_t *const out_ops_ = p.out_ops;        // (locals of the streaming loop, see the top of the kernel)
    const uint64_t slot_stride_ = p.slot_stride;
    const uint32_t brk_max_ = BRK ? p.brk_max : 0u;
    const int policy_ = p.policy, early_exit_ = p.early_exit, desc_mode_ = p.desc_mode;
    const uint64_t slot_row0 = 32ull * r + g0; // out_ops index of coordinate 0 in slot 0
    // first coordinate a clip of class k may start at in a later pass: behind every clip the earlier passes put there
    uint32_t carry[RB_MS];
#pragma unroll
    for (int q = 0; q < RB_MS; q++) carry[q] = 0u;

    const bool fused = p.fused != 0;
    uint32_t rec_nmatch = 0, rec_aln_len = 0; // of the whole (normalised) record: taken from its row, or from the fused verification
    if (!fused) rec_nmatch = nr->nmatch, rec_aln_len = nr->aln_len;
    uint64_t n_items = BRK ? 1 : ((nh == 0 && fused) ? 1 : nh); // (a record no window overlaps is still streamed once, to verify it; BRK: set by the first pass)
    // BRK, across passes: where the scratch rows of the record begin, and the cut state (pieces closed, end of the last long indel)
    // at the start of the segment in which the next pass's first piece opens
    uint64_t brk_row0 = 0;
    uint32_t brk_res_cnt = 0, brk_res_pre = 0;
    // where a later pass may start streaming: the segment in which the previous pass resolved the start of its last window
    // (windows are sorted, so nothing of the next pass lies before it), with the running totals at that point
    uint32_t resume_seg = 0, resume_R = 0, resume_Q = 0, resume_U = 0;
    unsigned long long sv_exec;
    asm volatile("s_mov_b64 %0, exec" : "=s"(sv_exec));
    const uint32_t lane_boff = (uint32_t)lane * 16u; // of the lane's group A in the step; group B lies 1024 bytes behind
    // (chunks past the record's end are not loaded: lanes behind the last chunk re-read it, and the loads of steps
    //  behind the last one run with an empty exec mask)
    // (the clamp is made per group -- the second group's address is the first one's plus 1024 only while neither is clamped --, so
    //  each load has an address register of its own where the stores, which are not clamped, use offset:1024)
#define RB_RING_LOAD_ASM(A, B_, C_, D_)                                                                                    \
    asm volatile("s_mov_b64 exec, %[lm]\n\t"                                                                                    \
         "global_load_dwordx4 " RB_RREG(A, 3) ", %[o], %[sb]\n\t"                                                       \
         "global_load_dwordx4 " RB_RREG(C_, 3) ", %[o2], %[sb]\n\t"                                                     \
         "s_mov_b64 exec, %[sv]"                                                                                        \
         :                                                                                                              \
         : [o] "v"(lo_), [o2] "v"(lo2_), [sb] "s"(gb_), [lm] "s"(lm_), [sv] "s"(sv_)                                    \
         : "memory", RB_RING_TOP);
#define RB_RING_LOAD(RING, STP)                                                                                                 \
    {                                                                                                                           \
        const uint32_t stp_ = (STP);                                                                                            \
        uint32_t lo_ = (stp_ << (RB_STEP_SHIFT + 2)) + lane_boff;                                                               \
        const uint32_t *const gb_ = gbase0; /* (named copies: a generic lambda does not capture what only an asm operand uses) */ \
        const unsigned long long sv_ = sv_exec;                                                                                 \
        const unsigned long long lm_ = stp_ < n_steps ? sv_ : 0ull;                                                             \
        uint32_t lo2_ = lo_ + 1024u;                                                                                            \
        lo_ = lo_ < last_boff ? lo_ : last_boff;                                                                                \
        lo2_ = lo2_ < last_boff ? lo2_ : last_boff;                                                                             \
        RB_RING_CASE(RING, RB_RING_LOAD_ASM)                                                                                    \
    }
#define RB_RING_NOSTORES                                                                                                        \
    _Pragma("unroll") for (int q_ = 0; q_ < RB_GRP * RB_MS; q_++)                                                               \
        asm volatile("s_mov_b64 exec, 0\n\tglobal_store_dword %0, %0, %1\n\ts_mov_b64 exec, %2" ::"v"(0u), "s"(gbase0), "s"(sv_exec) : "memory");
    // the capture's asm statements (the ring's registers named literally, like the loads and stores): the slot's last op into a register
    // of the compiler's; an entry of the capture table written from the slot; the last op of lane 63 into a scalar register
#define RB_RING_LASTOP(A, B_, C_, D_) asm volatile("v_mov_b32 %0, " RB_RREG1(D_) "\n\ts_nop 1" : "=v"(lastw));
    // (group A's last op; an entry's 16 bytes of ops from each lane of the pair, the rest from the even lane)
#define RB_RING_LASTOP_A(A, B_, C_, D_) asm volatile("v_mov_b32 %0, " RB_RREG1(B_) "\n\ts_nop 1" : "=v"(lastw_a));
#define RB_RING_CAPTURE_FLAT(G)                                                                                                 \
    asm volatile("s_mov_b64 exec, %[mp]\n\tds_write_b128 %[ea], " G "\n\ts_mov_b64 exec, %[me]\n\t"                            \
                 "ds_write2_b32 %[ea], %[pv], %[xr] offset0:8 offset1:9\n\tds_write2_b32 %[ea], %[xq], %[xu] offset0:10 offset1:11\n\t" \
                 "ds_write_b32 %[ta], %[tq]\n\ts_mov_b64 exec, %[sv]\n\ts_waitcnt lgkmcnt(0)"                                  \
                 :                                                                                                              \
                 : [ea] "v"(ea), [pv] "v"(pv_), [xr] "v"(xr_), [xq] "v"(xq_), [xu] "v"(xu_), [ta] "v"(ta), [tq] "v"(tq_),        \
                   [mp] "s"(mp_), [me] "s"(me_), [sv] "s"(sv_p)                                                                 \
                 : "memory");
#define RB_RING_CAPTURE_A(A, B_, C_, D_) RB_RING_CAPTURE_FLAT(RB_RREG(A, 3))
#define RB_RING_CAPTURE_B(A, B_, C_, D_) RB_RING_CAPTURE_FLAT(RB_RREG(C_, 3))
#define RB_RING_CARRY(A, B_, C_, D_) asm volatile("v_readlane_b32 %0, " RB_RREG1(D_) ", 63" : "=s"(v_carry));
    // The first pass of a record streams it from its first step: the ring's first loads go out HERE, in front of the pass's window loads
    // (a chain of dependent loads of its own), not behind them -- one memory latency per record instead of two in front of the first step.
    const bool preloaded = !(dbg & 4);
    if (preloaded) {
        __builtin_amdgcn_s_waitcnt(0x0F70); // vmcnt(0) (see the stream)
        RB_RING_LOAD(0, 0u)
        { RB_RING_NOSTORES }
        RB_RING_LOAD(1, 1u)
    }
    for (uint64_t jb = 0; jb < n_items; jb += RB_HMAX) {
        uint32_t nb = BRK ? 0u : (uint32_t)((nh - jb) < RB_HMAX ? (nh - jb) : RB_HMAX); // (BRK: pieces of this pass known so far, the open one included)
        const bool validate = fused && jb == 0;
        // ---- per-hit setup: lanes j and j + 32 both look at window jb + j; lane j resolves its start
        //      boundary, lane j + 32 its end boundary; lane j then owns the row ----
        const uint32_t hl = (uint32_t)lane & 31u;
        bool own = hl < nb;
        bool mine = own && lane < 32;
        const bool is_start = lane < 32;
        uint64_t wst = 0, wen = 0;
        uint32_t win = (uint32_t)jb + hl; // (BRK: the piece's ordinal)
        if constexpr (!BRK) {
            const rb_pass_win pw = rb_pass_windows(kp, &wx_all[wib][0], explicit_w, mono, ws, we, lo, h0, jb, nb, t_st, t_en, scan_pos, lane);
            wst = pw.wst, wen = pw.wen, win = pw.win;
        }
        const bool inside = !BRK && own && (t_st > wst && t_en < wen); // liftover.rs:23-25 (a piece never contains its record)
        // D = (relative ref offset of the boundary base) + 1
        uint32_t D = is_start ? (uint32_t)((wst > t_st ? wst : t_st) - t_st) + 1u // liftover.rs:28
                              : (uint32_t)((wen < t_en ? wen : t_en) - t_st);     // (min(en,t_en) - 1 - t_st) + 1, :38-40
        bool need = own && !inside;
        // BRK: piece j is the stretch from the end of a long indel (liftover.rs:203-206: pre_tpos) to the start of the next one
        // (cur_tpos, :190-201), kept if it holds reference bases; lane j carries its start, lane j + 32 its end, both as D above.
        // Piece brk_cnt is OPEN: its start is known (brk_pre), its end not yet (D = ~0 keeps it in every test below).
        // A pass takes pieces jb .. jb + 31; the first pass streams the whole record and counts all of them, a later one starts at
        // the segment in which its first piece opened (the cut state of that segment's start comes with it) and stops when its
        // pieces are closed and resolved.
        uint32_t brk_cnt = 0, brk_pre = 0;
        uint32_t brk_seg_cnt = 0, brk_seg_pre = 0; // ... at the start of the current segment
        uint32_t brk_nx_cnt = 0, brk_nx_pre = 0;   // ... of the segment the next pass resumes at
        unsigned long long brk_def = 0ull;         // lanes whose D is final
        const uint32_t brk_j0 = (uint32_t)jb;
        if constexpr (BRK) {
            if (jb != 0) brk_cnt = rb_first(brk_res_cnt), brk_pre = rb_first(brk_res_pre);
            D = 0xFFFFFFFFu;
            if (brk_cnt >= brk_j0 && brk_cnt - brk_j0 < 32u) { // the open piece is one of this pass's
                D = (uint32_t)lane == brk_cnt - brk_j0 ? brk_pre + 1u : D;
                brk_def = 1ull << (brk_cnt - brk_j0);
                nb = brk_cnt - brk_j0 + 1u;
            }
            need = false;
        }
        rb_bres O;
        O.st = RB_S_UNRES;
        O.op = O.part = O.R = O.Q = O.U = 0;
        if (dbg & 32) { // (the window values must have arrived for the phase boundary to mean anything)
            asm volatile("s_waitcnt vmcnt(0)");
        }
        RB_PHASE(0)
        // speculative emission: sorted windows only (the clips of a class then follow one another along the record)
        const bool spec = n_slots != 0u && mono && nb != 0u && !desc_mode_ && !(dbg & 1);
        const bool any_inside = __ballot(inside && mine) != 0; // (a clip that is the whole record needs the whole stream)
        const bool resumable = mono && jb != 0 && !any_inside; // later passes start where the previous one found its last start, and stop when done

        // ---- stream the record, RB_SMAX steps per segment; resolve after each segment ----
        uint32_t Rb = 0, Qb = 0, Ub = 0; // running totals
        uint32_t seg_first = 0;
        if (resumable) seg_first = resume_seg, Rb = resume_R, Qb = resume_Q, Ub = resume_U;
        if constexpr (BRK) // (set inside the step lambda: told to the compiler as the wave-uniform values they are)
            seg_first = rb_first(seg_first), Rb = rb_first(Rb), Qb = rb_first(Qb), Ub = rb_first(Ub);
        uint32_t next_seg = seg_first, next_R = Rb, next_Q = Qb, next_U = Ub; // resume point for the pass after this one
        // fused verification (first pass), per lane: AND of the "regular op" masks, minimum op word (below 16: a zero length),
        // minimum of code XOR previous code (0: two adjacent ops of one type), maximum of the per-lane length sums (2^25 and
        // more: the 64-lane scans could leave 32 bits; handed back like a zero length)
        uint32_t v_reg = 0xFFFFFFFFu, v_minw = 0xFFFFFFFFu, v_adj = 0xFFFFFFFFu, v_maxsu = 0u;
        uint32_t v_carry = 0xFu;       // last op word of the previous step (code 15: equals nothing; none yet)
        unsigned long long cap_mask = 0ull; // boundaries of this pass whose entry of the capture table is valid
        unsigned long long cap_pend = 0ull; // ... whose offset is the first one of the next step (their clip ended on the last base of this one)
        unsigned long long v_utot = 0; // 64-bit sum of all lengths
        const bool streams = BRK || ((__ballot(need) != 0 || validate || (spec && any_inside)) && !(dbg & 4));
        // diagnostics (dbg & 128): the clock this kernel holds while it streams -- s_memtime counts shader cycles, s_memrealtime a
        // constant 100 MHz -- stamped around the streaming loop of every 16th record, summed into counters->phase[0] (64 cycles) and
        // phase[1] (10 ns); phase[2] counts the stamped records.  Nothing reads these words on the device.
        unsigned long long ck_c0 = 0, ck_r0 = 0;
        if (dbg & 128) ck_c0 = __builtin_amdgcn_s_memtime(), ck_r0 = __builtin_amdgcn_s_memrealtime();
        if (streams) {
            // The load ring and the speculative stores are written by hand.  vmcnt retires in issue order on gfx9 and counts
            // loads and stores together; left to the compiler, the wait for a step's loads would also wait for the stores of
            // the step before (it sees only its own loads between a load and its use).  Every step issues exactly
            // RB_STEP_VMEM vector-memory instructions (stores of an empty mask and loads past the record's end are issued
            // with an empty exec mask), so "all but the youngest (RB_PF - 1) * RB_STEP_VMEM" is exactly "this step's loads
            // have landed".  Store data is read when the store issues: a ring slot is reloaded right behind its stores.
            // (a wait the compiler knows about: whatever load it still tracks as pending on a register the ring is about to
            //  take would otherwise cost an s_waitcnt vmcnt(0) inside the loop, on every step)
            __builtin_amdgcn_s_waitcnt(0x0F70); // vmcnt(0)
            if (!(preloaded && jb == 0)) {
            RB_RING_LOAD(0, seg_first * RB_SMAX)
            { RB_RING_NOSTORES }
            RB_RING_LOAD(1, seg_first * RB_SMAX + 1u)
            }
            // Speculative emission, per slot ("class") q: the CURRENT clip of the class -- its index among the pass's clips and its span in
            // reference offsets [c_ds, c_de) --, wave-uniform.  The clips of a class follow one another along the record (sorted windows),
            // so a step looks at the current clip and moves on only when that clip ends inside the step (round 3 kept a window [j_lo, j_hi)
            // over all classes and ran a scalar loop over it in every step: 60 of the step's 140 scalar instructions).
            uint32_t c_j[RB_MS], c_ds[RB_MS], c_de[RB_MS];
            auto clip_fetch = [&](const int q) { // (D lives in lanes: lane j the start of clip j, lane 32 + j its end)
                const bool ok = c_j[q] < nb;
                const uint32_t jj = ok ? c_j[q] : 0u;
                const uint32_t ds_ = rb_readlane<uint32_t>(D, (int)jj), de_ = rb_readlane<uint32_t>(D, (int)(32u + jj));
                c_ds[q] = ok ? ds_ : 0xFFFFFFFFu; // (no clip: a span no chunk reaches)
                c_de[q] = ok ? de_ : 0xFFFFFFFFu;
            };
#pragma unroll
            for (int q = 0; q < RB_MS; q++) { // clip j of the pass is of class (jb + j) mod n_slots
                const uint32_t ns_ = n_slots ? n_slots : 1u;
                c_j[q] = (uint32_t)q < n_slots ? ((uint32_t)q + ns_ - (uint32_t)(jb % ns_)) % ns_ : 0x7FFFFFFFu;
                clip_fetch(q);
            }
            uint32_t Rseg = 0, Qseg = 0, Useg = 0, seg0 = 0;
            // one step of the stream; EDGE = the record's first or last step (ops of the neighbours around it)
            // (a third form, the interior step of a first pass with its per-step tests folded to constants, lost: where it met the general
            //  form in one loop body the compiler moved two dozen values from one set of registers to another between steps)
            auto step = [&](auto ring_c, auto edge_c, const uint32_t st, const uint32_t seg1) {
                constexpr int ring = decltype(ring_c)::value;
                constexpr bool edge = decltype(edge_c)::value;
                // (the pass's flags as values of the step, not read through the lambda's references: spelled any other way the compiler's
                //  register assignment moves)
                const bool validate_s = validate, spec_s = spec, later_s = jb != 0;
                // the step's 8 ops leave the ring for registers of the compiler's choosing once they have landed
                // (no memory clobber: the compiler takes an asm that may load for a load still in flight and waits vmcnt(0) at the first use of its outputs)
                unsigned long long a0, a1, a2 = 0, a3 = 0;
#define RB_RING_TAKE(A, B_, C_, D_)                                                                                             \
    asm volatile("s_waitcnt vmcnt(%4)\n\t"                                                                                      \
                 "v_mov_b64 %0, " RB_RREG(A, 1) "\n\tv_mov_b64 %1, " RB_RREG(B_, 1) "\n\tv_mov_b64 %2, " RB_RREG(C_, 1) "\n\tv_mov_b64 %3, " RB_RREG(D_, 1) \
                 : "=v"(a0), "=v"(a1), "=v"(a2), "=v"(a3)                                                                       \
                 : "n"(RB_RING_WAIT));
                RB_RING_CASE(ring, RB_RING_TAKE)
#undef RB_RING_TAKE
                unsigned long long msk[RB_MS], mskb[RB_MS]; // lanes whose group A / group B may hold ops of the slot's clips
#pragma unroll
                for (int q = 0; q < RB_MS; q++) msk[q] = mskb[q] = 0ull;
                if (st < seg1) { // (no break: the ring must be in the same state on every path)
                    static_assert(RB_OPL == 8, "two groups of four ops");
                    // the lane's ops: w[0..3] group A (ops 4 l .. of the step's first half), w[4..7] group B (the same of its second half)
                    uint32_t w[RB_OPL] = {(uint32_t)a0, (uint32_t)(a0 >> 32), (uint32_t)a1, (uint32_t)(a1 >> 32),
                                          (uint32_t)a2, (uint32_t)(a2 >> 32), (uint32_t)a3, (uint32_t)(a3 >> 32)};
                    uint32_t c[RB_OPL]; // what the verification looks at
#pragma unroll
                    for (int q = 0; q < RB_OPL; q++) c[q] = w[q];
                    if (edge) {
                        // ops of the neighbouring records: zero for the sums (a 0-length M); for the verification an I / D of length
                        // 1 by position parity -- regular, alternating, and never equal to the match op a normalised record ends on.
                        // Each group by its own index.
                        const int32_t idx0 = (int32_t)(st << RB_STEP_SHIFT) + lane * 4 - head;
#pragma unroll
                        for (int q = 0; q < RB_OPL; q++) {
                            const bool ok = (uint32_t)(idx0 + (q & 3) + (q >> 2) * 256) < n;
                            c[q] = ok ? w[q] : ((q & 1) ? 0x12u : 0x11u);
                            w[q] = ok ? w[q] : 0u;
                        }
                    }
                    if (validate_s) {
                        // the op in front of a group: the lane below's last op of the same half; lane 0 of B: lane 63's last op of A; lane 0
                        // of A: the last op of the step before
                        const uint32_t prev_a = rb_prev_lane(c[3], v_carry), prev_b = rb_prev_lane(c[7], rb_readlane<uint32_t>(c[3], 63));
                        uint32_t rg[RB_OPL], x[RB_OPL];
#pragma unroll
                        for (int q = 0; q < RB_OPL; q++) {
                            rg[q] = (uint32_t)__builtin_amdgcn_sbfe((int)0x018F018Fu, c[q], 1u); // M I D N = X
                            x[q] = (c[q] ^ (q == 0 ? prev_a : (q == 4 ? prev_b : c[q - 1]))) & 15u;
                        }
                        auto min3 = [](uint32_t a, uint32_t b, uint32_t d) { const uint32_t t = a < b ? a : b; return t < d ? t : d; };
#pragma unroll
                        for (int q = 0; q < RB_OPL; q += 2) {
                            v_reg &= rg[q] & rg[q + 1];
                            v_minw = min3(v_minw, c[q], c[q + 1]);
                            v_adj = min3(v_adj, x[q], x[q + 1]);
                        }
                    }
                    // per-lane sums of the reference / query / unit lengths of each group's 4 ops; regular records hold only
                    // M I D N = X, so "consumes the reference" = not I and "consumes the query" = not D / N: one
                    // v_bfe_i32 per class turns the op code (low bits of the word) into an all-ones / zero mask.
                    // A's sums are scanned across the wave, B's on top of A's totals.
                    uint32_t sr = 0, sq = 0, su = 0, srb = 0, sqb = 0, sub = 0;
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const uint32_t len = rb_len(w[q]), lenb = rb_len(w[4 + q]);
                        sr += len & (uint32_t)__builtin_amdgcn_sbfe((int)0xFFFDFFFDu, w[q], 1u);
                        sq += len & (uint32_t)__builtin_amdgcn_sbfe((int)0xFFF3FFF3u, w[q], 1u); // not D, not N
                        su += len;
                        srb += lenb & (uint32_t)__builtin_amdgcn_sbfe((int)0xFFFDFFFDu, w[4 + q], 1u);
                        sqb += lenb & (uint32_t)__builtin_amdgcn_sbfe((int)0xFFF3FFF3u, w[4 + q], 1u);
                        sub += lenb;
                    }
                    const uint32_t R0 = Rb;
                    const uint32_t ir = rb_wave_scan_incl(sr), iq = rb_wave_scan_incl(sq), iu = rb_wave_scan_incl(su);
                    const uint32_t irb = rb_wave_scan_incl(srb) + rb_readlane<uint32_t>(ir, 63), iqb = rb_wave_scan_incl(sqb) + rb_readlane<uint32_t>(iq, 63),
                                   iub = rb_wave_scan_incl(sub) + rb_readlane<uint32_t>(iu, 63);
                    // exclusive prefixes in front of each group: the checkpoints, and what a captured boundary takes along
                    const uint32_t cR = R0 + ir - sr, cE = R0 + ir, xQ = Qb + iq - sq, xU = Ub + iu - su;
                    const uint32_t cRb = R0 + irb - srb, cEb = R0 + irb, xQb = Qb + iqb - sqb, xUb = Ub + iub - sub;
                    constexpr uint32_t LPC = CPO / 4u; // lanes of a half per checkpoint
                    if (((uint32_t)lane & (LPC - 1u)) == 0u) { // a checkpoint every CPO ops, in op order: half A's, then half B's
                        const uint32_t t = (st - seg0) * CPS + (uint32_t)lane / LPC;
                        cpR[t] = cR, cpQ[t] = xQ, cpU[t] = xU;
                        cpR[t + CPS / 2u] = cRb, cpQ[t + CPS / 2u] = xQb, cpU[t + CPS / 2u] = xUb;
                    }
                    Rb += rb_readlane<uint32_t>(irb, 63); // (A + B: B's sums are scanned on top of A's totals)
                    Qb += rb_readlane<uint32_t>(iqb, 63);
                    Ub += rb_readlane<uint32_t>(iub, 63);
                    if (validate_s) {
                        // (the guard stays what it was, the sum of 8 ops aligned to 8: a lane's group and its pair lane's, quad_perm [1 0 3 2])
                        const uint32_t pa = su + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)su, 0xB1, 0xf, 0xf, false);
                        const uint32_t pb = sub + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)sub, 0xB1, 0xf, 0xf, false);
                        const uint32_t sm = pa > pb ? pa : pb;
                        v_maxsu = v_maxsu > sm ? v_maxsu : sm;
                        v_utot += rb_readlane<uint32_t>(iub, 63);
                    }
                    if constexpr (BRK) {
                        // long indels among my 8 ops (ops of the neighbouring records are zero words here: an M of length 0).  They are
                        // rare -- one step in six has one -- and are taken one by one, in op order (the lanes of half A, then those of
                        // half B), with wave-uniform arithmetic
                        bool big_a = false, big_b = false;
#pragma unroll
                        for (int q = 0; q < 4; q++) {
                            const uint32_t ca = w[q] & 15u, cb = w[4 + q] & 15u;
                            big_a |= (ca == RB_OP_I || ca == RB_OP_D) && rb_len(w[q]) > brk_max_;
                            big_b |= (cb == RB_OP_I || cb == RB_OP_D) && rb_len(w[4 + q]) > brk_max_;
                        }
                        const unsigned long long cm_a = __ballot(big_a), cm_b = __ballot(big_b);
                        const bool had_big = (cm_a | cm_b) != 0ull;
                        rb_static_for<2>([&](auto half_c) {
                            constexpr int hb = decltype(half_c)::value;
                            unsigned long long cm = hb ? cm_b : cm_a;
                            while (cm) {
                                const int l = __builtin_ctzll(cm);
                                cm &= cm - 1ull;
                                uint32_t rx = rb_readlane<uint32_t>(hb ? cRb : cR, l); // reference offset of the group's first op
#pragma unroll
                                for (int q = 0; q < 4; q++) {
                                    const uint32_t wq = rb_readlane<uint32_t>(w[4 * hb + q], l);
                                    const uint32_t cq = wq & 15u, lq = rb_len(wq);
                                    const uint32_t rlq = cq == RB_OP_I ? 0u : lq; // (regular records: M I D N = X)
                                    if ((cq == RB_OP_I || cq == RB_OP_D) && lq > brk_max_) {
                                        if (rx > brk_pre) { // liftover.rs:191: the piece in front of the indel, if it holds reference bases
                                            const uint32_t li = brk_cnt - brk_j0; // (its lane in this pass; wraps far above 32 for earlier pieces)
                                            if (li < 32u) {
                                                D = (uint32_t)lane == 32u + li ? rx : D;
                                                brk_def |= 1ull << (32u + li);
                                            }
                                            brk_cnt++;
                                            if (brk_cnt == brk_j0 + 32u) // the next pass's first piece opens in this segment: it resumes here
                                                next_seg = seg0 / RB_SMAX, next_R = Rseg, next_Q = Qseg, next_U = Useg, brk_nx_cnt = brk_seg_cnt, brk_nx_pre = brk_seg_pre;
                                        }
                                        brk_pre = rx + rlq; // :203-206
                                        {
                                            const uint32_t li = brk_cnt - brk_j0;
                                            if (li < 32u) { // the next piece opens here (its lanes are rewritten if it turns out empty)
                                                D = (uint32_t)lane == li ? brk_pre + 1u : ((uint32_t)lane == 32u + li ? 0xFFFFFFFFu : D);
                                                brk_def |= 1ull << li;
                                                brk_def &= ~(1ull << (32u + li));
                                            }
                                        }
                                    }
                                    rx += rlq;
                                }
                            }
                        });
                        nb = brk_cnt < brk_j0 ? 0u : (brk_cnt - brk_j0 + 1u < 32u ? brk_cnt - brk_j0 + 1u : 32u);
                        if (had_big) { // pieces were closed / opened: the classes' current clips are read again
#pragma unroll
                            for (int q = 0; q < RB_MS; q++) clip_fetch(q);
                        }
                    }
                    if (spec_s) {
                        // Which of a group's 4 ops a clip keeps is not known yet (boundaries are resolved per segment), but which
                        // groups can hold ops of clip j is: those whose reference span [cR, cE) reaches from the clip's first base
                        // (D_start - 1) to its last one (D_end - 1); walking to the next / previous match op only shrinks a clip.
                        // Those groups are stored as they are -- what lies outside the clip is never read, and the two end ops are
                        // rewritten with the clipped lengths once the boundaries are resolved.
                        // Capture: the group that holds a clip's start offset / its end offset (cR <= D < cE; at most one lane of one
                        // half) is in the 8 ops the resolution will search: the groups of the lane pair (l & ~1, l | 1) of that half.
                        // Under a mask that is empty in most steps both lanes write their 16 bytes of the boundary's entry (is / ie: the
                        // boundary's lane) straight from the ring, the even lane the op in front of its group, its prefixes and the
                        // chunk's number in the segment.
                        auto capture = [&](const bool hs, const bool hsb, const uint32_t is, const bool he, const bool heb, const uint32_t ie) {
                            const unsigned long long bs = rb_ballot(hs), bsb = rb_ballot(hsb), be = rb_ballot(he), beb = rb_ballot(heb);
                            if ((bs | bsb | be | beb) != 0ull) {
                                uint32_t lastw_a, lastw;
                                RB_RING_CASE(ring, RB_RING_LASTOP_A)
                                RB_RING_CASE(ring, RB_RING_LASTOP)
                                const uint32_t pv_a = rb_prev_lane(lastw_a, v_carry), pv_b = rb_prev_lane(lastw, rb_readlane<uint32_t>(lastw_a, 63));
                                // (lane 0 of the step a later pass resumes at has no op in front: the fallback takes the boundaries of its pair)
                                const bool pv_ok = st == 0u || v_carry != 0xFu;
                                auto pair = [](unsigned long long m) { m = (m | (m >> 1)) & 0x5555555555555555ull; return m | (m << 1); };
                                const unsigned long long ps = pair(bs) & (pv_ok ? ~0ull : ~3ull), pe = pair(be) & (pv_ok ? ~0ull : ~3ull), psb = pair(bsb), peb = pair(beb);
                                const uint32_t wv = threadIdx.x >> 6;
                                const uint32_t tq_a = (st - seg0) * 64u + ((uint32_t)lane >> 1), tq_b = tq_a + 32u;
                                const uint32_t odd = ((uint32_t)lane & 1u) * 16u;
                                const unsigned long long sv_c = sv_exec;
                                auto put = [&](const uint32_t bi, const unsigned long long ma, const unsigned long long mb) {
                                    const unsigned long long sv_p = sv_c; // (named copies, see RB_RING_LOAD)
                                    const uint32_t ea = rb_lds_addr(&cap_all[0][0]) + (wv * 64u + bi) * 48u + odd, ta = rb_lds_addr(&cap_t[0][0]) + (wv * 64u + bi) * 4u;
                                    if (ma != 0ull) {
                                        const unsigned long long mp_ = ma, me_ = ma & 0x5555555555555555ull;
                                        const uint32_t pv_ = pv_a, xr_ = cR, xq_ = xQ, xu_ = xU, tq_ = tq_a;
                                        RB_RING_CASE(ring, RB_RING_CAPTURE_A)
                                    } else if (mb != 0ull) {
                                        const unsigned long long mp_ = mb, me_ = mb & 0x5555555555555555ull;
                                        const uint32_t pv_ = pv_b, xr_ = cRb, xq_ = xQb, xu_ = xUb, tq_ = tq_b;
                                        RB_RING_CASE(ring, RB_RING_CAPTURE_B)
                                    }
                                };
                                put(is, ps, psb);
                                put(ie, pe, peb);
                                cap_mask |= ((ps | psb) != 0ull ? 1ull << is : 0ull) | ((pe | peb) != 0ull ? 1ull << ie : 0ull);
                            }
                        };
                        // boundaries of clips that ended on the last base of the step before: their offset is this step's first one,
                        // held by the first chunk of half A that is not empty
                        if constexpr (CAP) {
                            while (cap_pend != 0ull) {
                                const uint32_t bi = (uint32_t)__builtin_ctzll(cap_pend);
                                cap_pend &= cap_pend - 1ull;
                                capture(cR == R0 && cE != R0, false, bi, false, false, bi);
                            }
                        }
#pragma unroll
                        for (int q = 0; q < RB_MS; q++) {
                            unsigned long long mk = 0ull, mkb = 0ull;
                            for (;;) {
                                mk |= rb_ballot(cR < c_de[q] && cE >= c_ds[q]);
                                mkb |= rb_ballot(cRb < c_de[q] && cEb >= c_ds[q]);
                                if constexpr (CAP)
                                    capture(c_ds[q] - cR < cE - cR, c_ds[q] - cRb < cEb - cRb, c_j[q] & 31u, c_de[q] - cR < cE - cR, c_de[q] - cRb < cEb - cRb, 32u + (c_j[q] & 31u));
                                if (c_de[q] > Rb) break; // the clip reaches past this step (or there is none): it stays the current one
                                // its last base is the step's last one: the chunk with its end offset is the next step's first
                                if (CAP && c_de[q] == Rb) cap_pend |= (1ull << (32u + (c_j[q] & 31u))) | (c_ds[q] == Rb ? 1ull << (c_j[q] & 31u) : 0ull);
                                c_j[q] += n_slots;       // it ends in this step: the class's next clip may begin in it
                                clip_fetch(q);
                                if (c_j[q] >= nb) break;
                            }
                            msk[q] = mk, mskb[q] = mkb;
                        }
                    }
                }
                // ---- stores of this step (always 2 * RB_MS instructions), then the slot's next loads ----
                {
                    const uint32_t so = (st << (RB_STEP_SHIFT + 2)) + lane_boff;
                    const unsigned long long sv_st = sv_exec;
                    unsigned long long v0 = sv_st, v1 = sv_st;
                    constexpr uint32_t so1 = 1024u, co1 = 256u; // the lane's group B behind its group A: bytes, ops
                    if (edge) { // groups in front of the record's first and behind its last one are not this record's to write
                        v0 = rb_ballot(so + 16u > first_boff && so <= last_boff);
                        v1 = rb_ballot(so + so1 + 16u > first_boff && so + so1 <= last_boff);
                    }
#pragma unroll
                    for (int q = 0; q < RB_MS; q++) {
                        const unsigned long long msk1 = mskb[q];
                        unsigned long long m0 = msk[q] & v0, m1 = msk1 & v1;
                        if (later_s && (msk[q] | msk1) != 0ull) { // later passes stay clear of the end ops earlier passes have patched
                            const uint32_t c0 = (st << RB_STEP_SHIFT) + (uint32_t)lane * 4u;
                            m0 &= rb_ballot(c0 >= carry[q]);
                            m1 &= rb_ballot(c0 + co1 >= carry[q]);
                        }
                        // The stores are widened to whole granules of 64 bytes (RB_GRAN ops, four lanes of one half): a lane in front of a clip's first group
                        // or behind its last one, in the same granule, stores what it loaded too (the record's own neighbouring ops; a slot's
                        // lines are this record's alone and nobody reads a slot outside a clip), and no two clips of a slot may share a granule
                        // instead of a 16-byte group.  Fewer lines written in part: -0.6 % on a fast box, -1.7 % on a slow one (r04_ab7, r04_hs8;
                        // a launch that writes no partial line at all is 5 % / 11 % shorter, profiles/r04_stream_summary.md).
                        if constexpr (!BRK) { // the granule is four lanes of one half (break-paf's pieces lie op to op: its groups stay 16 bytes)
                            auto gran = [](unsigned long long m) {
                                m |= m >> 1;
                                m = (m | (m >> 2)) & 0x1111111111111111ull;
                                m |= m << 1;
                                return m | (m << 2);
                            };
                            const unsigned long long keep0 = m0 | ~msk[q], keep1 = m1 | ~msk1; // (what the edge / carry filters took away stays away)
                            m0 = gran(m0) & keep0;
                            m1 = gran(m1) & keep1;
                        }
                        if (dbg & 64) m0 = m1 = 0ull; // diagnostics: everything but the stores themselves
                        const uint32_t *sb = out_ops_ + slot_row0 + (uint64_t)q * slot_stride_;
                        // (plain stores: nothing in this kernel is read twice any more, and non-temporal stores take 2 ms longer here)
#define RB_RING_STORE(A, B_, C_, D_)                                                                                            \
    asm volatile("s_mov_b64 exec, %[m0]\n\t"                                                                                    \
                 "global_store_dwordx4 %[o], " RB_RREG(A, 3) ", %[sb]\n\t"                                                      \
                 "s_mov_b64 exec, %[m1]\n\t"                                                                                    \
                 "global_store_dwordx4 %[o], " RB_RREG(C_, 3) ", %[sb] offset:%[o1]\n\t"                                        \
                 "s_mov_b64 exec, %[sv]"                                                                                        \
                 :                                                                                                              \
                 : [m0] "s"(m0), [m1] "s"(m1), [o] "v"(so), [sb] "s"(sb), [sv] "s"(sv_st), [o1] "n"(so1)                        \
                 : "memory");
                        RB_RING_CASE(ring, RB_RING_STORE)
#undef RB_RING_STORE
                    }
                }
                // the last op of the step, for the adjacency check and the captures of the next one (in front of the slot's reload).  The raw
                // word of lane 63, where the adjacency check used to carry its masked copy: they differ only when lane 63 lies past the
                // record's end, and no step follows such a step.  (An SGPR written inside an asm: the compiler's hazard recogniser does not
                // see the v_readlane, which is fine for VALU data -- never use v_carry as an address or a lane select.)
                RB_RING_CASE(ring, RB_RING_CARRY)
                RB_RING_LOAD(ring, st + RB_PF)
            };
            for (seg0 = seg_first * RB_SMAX; seg0 < n_steps; seg0 += RB_SMAX) {
                const uint32_t seg1 = (seg0 + RB_SMAX < n_steps) ? seg0 + RB_SMAX : n_steps;
                Rseg = Rb, Qseg = Qb, Useg = Ub;
                if constexpr (BRK) brk_seg_cnt = brk_cnt, brk_seg_pre = brk_pre;
                // the ring is indexed statically (unrolled by RB_PF): rotating it with register moves would make
                // every step wait for ALL loads in flight (the moves read their destination registers)
                for (uint32_t st0 = seg0; st0 < seg1; st0 += RB_PF) {
                    rb_static_for<RB_PF>([&](auto ring_c) {
                        const uint32_t st = st0 + (uint32_t)decltype(ring_c)::value;
                        if (st == 0 || st + 1 >= n_steps) step(ring_c, std::true_type{}, st, seg1);
                        else step(ring_c, std::false_type{}, st, seg1);
                    });
                }
                // ---- lane-parallel resolution of the boundaries that fall in this segment ----
                const bool last_seg = seg1 == n_steps;
                const uint32_t n_cp = (seg1 - seg0) * CPS;
                const int32_t cp_idx0 = (int32_t)(seg0 << RB_STEP_SHIFT) - head; // op index of checkpoint 0
                if constexpr (BRK) {
                    if (last_seg) { // liftover.rs:213-224: what lies behind the last long indel
                        const uint32_t li = brk_cnt - brk_j0;
                        if (Rb > brk_pre) {
                            if (li < 32u) {
                                D = (uint32_t)lane == 32u + li ? Rb : D;
                                brk_def |= 1ull << (32u + li);
                            }
                            brk_cnt++;
                        } else if (li < 32u) {
                            brk_def &= ~(1ull << li); // the record ends with a long indel: no piece was open after all
                        }
                    }
                    need = ((brk_def >> lane) & 1ull) != 0ull && O.st == RB_S_UNRES;
                }
                {
                    const bool todo = need && D >= Rseg && (D < Rb || (last_seg && D == Rb));
                    if (todo && !(dbg & 2)) {
                        if (D == Rb) { // boundary on the record's last base; the last op is match-type
                            const uint32_t lv = rec_ops[n - 1];
                            O.st = RB_S_OK, O.op = n - 1;
                            if (is_start) O.part = rb_part_pack(1u, lv), O.R = Rb - 1, O.Q = Qb - 1, O.U = Ub - 1;
                            else O.part = rb_part_pack(rb_len(lv), lv), O.R = Rb, O.Q = Qb, O.U = Ub;
                        } else {
                            // the group of 8 ops that holds offset D, the op in front of it and the prefixes at its first op: from the
                            // boundary's entry of the capture table, or -- a boundary no step captured: windows that are not sorted, a clip
                            // that starts in front of the step in which it became its class's current one, a later pass's resume point --
                            // from the last checkpoint with R <= D (R is non-decreasing) and the record
                            uint32_t g[8], pv, gR, gQ, gU;
                            int32_t gidx;
                            bool captured = false;
                            if constexpr (CAP) captured = ((cap_mask >> lane) & 1ull) != 0ull;
                            if (captured) {
                                const uint4 *e = &cap_all[wib][3 * lane];
                                const uint4 e0 = e[0], e1 = e[1], e2 = e[2];
                                g[0] = e0.x, g[1] = e0.y, g[2] = e0.z, g[3] = e0.w, g[4] = e1.x, g[5] = e1.y, g[6] = e1.z, g[7] = e1.w;
                                pv = e2.x, gR = e2.y, gQ = e2.z, gU = e2.w;
                                gidx = cp_idx0 + (int32_t)(cap_t[wib][lane] * RB_CP_OPS);
                                if (dbg & 1024) atomicAdd(&p.counters->phase[1], 1u); // diagnostics: boundaries resolved from their entry
                            } else {
                                uint32_t lo_t = 0, hi_t = n_cp;
                                while (hi_t - lo_t > 1) {
                                    const uint32_t mid = (lo_t + hi_t) >> 1;
                                    if (cpR[mid] <= D) lo_t = mid; else hi_t = mid;
                                }
                                gidx = cp_idx0 + (int32_t)(lo_t * CPO), gR = cpR[lo_t], gQ = cpQ[lo_t], gU = cpU[lo_t];
                                if constexpr (CAP) {
                                    rb_load_group_wide(rec_ops, n, gidx, gR, gQ, gU, D, g, pv);
                                } else {
                                    const uint4 *q = reinterpret_cast<const uint4 *>(rec_ops + gidx); // 16-byte aligned by construction
                                    const uint4 a0 = q[0], a1 = q[1];
                                    g[0] = a0.x, g[1] = a0.y, g[2] = a0.z, g[3] = a0.w, g[4] = a1.x, g[5] = a1.y, g[6] = a1.z, g[7] = a1.w;
                                    pv = rec_ops[gidx > 0 ? gidx - 1 : 0];
                                }
                                if (dbg & 1024) atomicAdd(&p.counters->phase[0], 1u); // diagnostics: ... from the checkpoints and the record
                            }
                            O = rb_resolve_group(rec_ops, n, gidx, g, pv, gR, gQ, gU, D, is_start, policy_);
                        }
                        need = false;
                    }
                    // (the group loads above may still be tracked as pending where a lane left rb_resolve early; the compiler
                    //  would then wait vmcnt(0) at the first write to one of their registers, which is inside the step loop.
                    //  The resolving lanes have waited for those loads -- the youngest in the queue -- anyway.)
                    __builtin_amdgcn_s_waitcnt(0x0F70); // vmcnt(0)
                    // the start of the pass's last window was found in this segment: the next pass begins here
                    if (!BRK && nb && ((__ballot(todo) >> (nb - 1u)) & 1ull)) next_seg = seg0 / RB_SMAX, next_R = Rseg, next_Q = Qseg, next_U = Useg;
                }
                if (!BRK && (early_exit_ || resumable) && !validate && !(spec && any_inside) && __ballot(need) == 0) break;
                if constexpr (BRK) { // a later pass is done when its 32 pieces are closed and every boundary of theirs is resolved
                    if (jb != 0 && brk_cnt >= brk_j0 + 32u && __ballot(((brk_def >> lane) & 1ull) != 0ull && O.st == RB_S_UNRES) == 0ull) break;
                }
            }
            // nothing of the ring may still be in flight when its registers go back to the compiler (a pass that leaves early
            // has loads out), and the end ops below must land after the speculative stores to the same addresses
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#undef RB_RING_LOAD
#undef RB_RING_LOAD_ASM
#undef RB_RING_LASTOP_A
#undef RB_RING_CAPTURE_FLAT
#undef RB_RING_NOSTORES
#undef RB_RING_LASTOP
#undef RB_RING_CAPTURE_A
#undef RB_RING_CAPTURE_B
#undef RB_RING_CARRY
        }
        if (!streams && preloaded && jb == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // (the ring's loads are out: nothing of them may be in flight when the registers are the compiler's again)
        if (dbg & 128) {
            const unsigned long long ck_c1 = __builtin_amdgcn_s_memtime(), ck_r1 = __builtin_amdgcn_s_memrealtime();
            if (lane == 0 && (wave & 15) == 0) {
                atomicAdd(&p.counters->phase[0], (uint32_t)((ck_c1 - ck_c0) >> 6));
                atomicAdd(&p.counters->phase[1], (uint32_t)(ck_r1 - ck_r0));
                atomicAdd(&p.counters->phase[2], 1u);
            }
        }
        resume_seg = next_seg, resume_R = next_R, resume_Q = next_Q, resume_U = next_U;
        kq = rb_kp_here(kp); // (what the rows, patches and lists below need is loaded from here on, not carried through the stream)
        // ---- behind the stream.  What this part needs to know about the record it reads again from the job (64 bytes at an address
        //      the whole wave shares, L2-resident) and derives afresh: computed in front of the stream these values -- row and slot
        //      addresses, flags, counts -- were carried through it in scalar registers the streaming loop has no room for, i.e.
        //      spilled (round 2: 233 spills) ----
        const rb_job jp = p.jobs[wave];
        if constexpr (coord_reload) t_st = jp.t_st, t_en = jp.t_en, q_st = jp.q_st, q_en = jp.q_en;
        {
        const uint32_t r = rb_first(jp.r), n = rb_first(jp.n);
        const rb_norm_row *nr = &p.norm[r];
        const uint64_t rec0 = rb_first64(jp.rec0);
        const uint32_t *rec_ops = p.ops + rec0;
        const int32_t head = (int32_t)(rec0 & 31ull);
        const uint64_t slot_row0 = 32ull * r + (rec0 & ~31ull);
        const uint64_t h0 = rb_first(jp.h0), nh = rb_first(jp.nh);
        const bool minus = (rb_first(jp.flags) & RB_JOB_MINUS) != 0;

        RB_PHASE(1)
        if (validate) {
            // ---- the verdict of the fused scan: check_integrity (paf.rs:825-857) on the normalised record and the
            //      conditions of the fast path.  A record that fails any of them is handed back: the full record scan
            //      (list mode) decides its status, the generic kernel clips it if it is merely irregular ----
            const bool lane_bad = v_reg != 0xFFFFFFFFu || v_minw < 16u || v_adj == 0u || (v_maxsu >> 25) != 0u;
            const bool bad = __ballot(lane_bad) != 0 || rb_first64(v_utot) > 0xFFFFFFFFull || t_en < t_st || q_en < q_st ||
                             (uint64_t)Rb != t_en - t_st || (uint64_t)Qb != q_en - q_st;
            if (bad) {
                if (lane == 0) {
                    const unsigned long long i = atomicAdd(p.pend_count, 1ull);
                    p.pend_list[i] = r;
                }
                if constexpr (BRK) {
                    brk_decline();
                    return;
                }
                if (!BRK && nh) {
                    if (!explicit_w) {
                        const uint32_t cg = p.contig[r];
                        ws = p.cw_off[cg];
                        we = p.cw_off[cg + 1];
                    }
                    rb_defer_record(kp, r, nr, h0, nh, explicit_w, mono, ws, we, lane);
                }
                return;
            }
            rec_nmatch = Rb + Qb - Ub; // match units = ref + query - all (M I D = X only)
            rec_aln_len = Ub;
            if (lane == 0) { // (RB_F_HAS_M is reported by rb_dev_scan_records only: nothing on this path reads it)
                rb_norm_row *w = &p.norm_w[r];
                w->nmatch = rec_nmatch;
                w->aln_len = rec_aln_len;
                w->flags = (nr->flags & RB_F_STRIPPED) | RB_F_REGULAR;
            }
            if (!BRK && nh == 0) { // (no window overlaps the record: it has been walked and verified, liftover.rs:119-121, and that is all)
                if ((dbg & 256) && lane == 0) p.diag_stamps[wave] = (uint32_t)__builtin_amdgcn_s_memrealtime();
                return;
            }
        }
        if constexpr (BRK) {
            brk_cnt = rb_first(brk_cnt), brk_nx_cnt = rb_first(brk_nx_cnt), brk_nx_pre = rb_first(brk_nx_pre);
            if (jb == 0) {
                // the first pass has seen every piece.  Rows: a place for all of them from one of the bump cursors (one atomic per
                // record; a single cursor would serialise the records at one L2 line), the count for the scan that orders the rows
                n_items = brk_cnt;
                unsigned long long b0 = 0;
                const uint32_t ar = (uint32_t)(wave % p.brk_n_arena);
                if (lane == 0 && brk_cnt) b0 = atomicAdd(&p.brk_cursor[(size_t)ar * 16u], (unsigned long long)brk_cnt);
                b0 = rb_first64(b0);
                if (b0 + brk_cnt > p.brk_arena_cap) { // (this cursor's share of the scratch rows is used up: rb_k_finish asks for more rows)
                    if (lane == 0) p.counters->brk_scratch_short = 1, p.hit_off[r] = brk_cnt, p.brk_off[r] = ~0ull;
                    return;
                }
                brk_row0 = (uint64_t)ar * p.brk_arena_cap + b0;
                if (lane == 0) p.hit_off[r] = brk_cnt, p.brk_off[r] = brk_row0;
                if (brk_cnt == 0) return;
            }
            nb = (uint32_t)(n_items - jb < 32u ? n_items - jb : 32u);
            own = hl < nb, mine = own && lane < 32;
            brk_res_cnt = brk_nx_cnt, brk_res_pre = brk_nx_pre;
        }
        // ---- finalize: lane j (< 32) computes the row of hit jb + j; the end comes from lane j + 32 ----
        const rb_bres A = O;
        rb_bres B;
        B.st = (uint32_t)__shfl((int)O.st, lane + 32, 64);
        B.op = (uint32_t)__shfl((int)O.op, lane + 32, 64);
        B.part = (uint32_t)__shfl((int)O.part, lane + 32, 64);
        B.R = (uint32_t)__shfl((int)O.R, lane + 32, 64);
        B.Q = (uint32_t)__shfl((int)O.Q, lane + 32, 64);
        B.U = (uint32_t)__shfl((int)O.U, lane + 32, 64);
        uint32_t status = RB_ST_OK, out_n = 0, a_op = 0;
        uint64_t o_tst = 0, o_ten = 0, o_qst = 0, o_qen = 0;
        uint32_t o_nm = 0, o_al = 0;
        bool defer = false;
        if (mine) {
            if (inside) {
                out_n = n;
                o_tst = t_st, o_ten = t_en, o_qst = q_st, o_qen = q_en;
                o_nm = rec_nmatch, o_al = rec_aln_len;
            } else if (A.st == RB_S_DEFER || B.st == RB_S_DEFER || A.st == RB_S_UNRES || B.st == RB_S_UNRES) {
                defer = true;
            } else if (A.st == RB_S_NONE || B.st == RB_S_NONE || A.U >= B.U) {
                status = RB_ST_NONE_INDEL; // liftover.rs:52-54
            } else {
                a_op = A.op;
                o_tst = t_st + A.R; // liftover.rs:57-60, :77-82
                o_ten = t_st + B.R;
                if (!minus) {
                    o_qst = q_st + A.Q;
                    o_qen = q_st + B.Q;
                } else {
                    o_qst = q_en - B.Q;
                    o_qen = q_en - A.Q;
                }
                o_al = B.U - A.U;
                o_nm = (B.R + B.Q - B.U) - (A.R + A.Q - A.U); // match units = ref + query - all (M I D = X only)
                out_n = B.op - A.op + 1;
            }
        }
        if constexpr (BRK) { // a boundary only the generic kernel resolves (it wants the piece's window in its row's place): the whole record goes
            if (__ballot(mine && defer) != 0ull) {
                brk_decline();
                return;
            }
        }
        const bool emits = mine && !defer && status == RB_ST_OK && !desc_mode_;
        const uint32_t e_first = (uint32_t)head + a_op; // coordinate (op index + head, counted from the aligned g0) of the first op
        const uint32_t e_cnt = emits ? out_n : 0u;
        const uint32_t eg_last = e_first + e_cnt - 1u;
        constexpr uint32_t gran = BRK ? 4u : (uint32_t)RB_GRAN; // ops per group no two clips of a slot may share
        const uint32_t eg_f = e_first & ~(gran - 1u), eg_l = e_cnt ? (eg_last & ~(gran - 1u)) : eg_f;
        // ---- which clips own their place in a slot.  Clip j (class j mod n_slots) does when it starts behind the last group
        //      of every earlier clip of its class: then no two clips of a slot share a 16-byte group, and the groups a clip
        //      rewrites (its first and last) are nobody else's.  With windows that overlap at most n_slots deep that is every
        //      clip; the others are copied to the arena area by rb_k_copy_clips. ----
        const uint32_t ns1 = n_slots ? n_slots : 1u;
        const uint32_t cls = (uint32_t)((jb + hl) % ns1);
        const uint32_t lgp = (emits && e_cnt) ? eg_l + gran : 0u; // first coordinate behind my clip's last group (0: no clip)
        uint32_t pm = lane < 32 ? lgp : 0u;                      // inclusive prefix maximum over the lanes of my class
        for (uint32_t d = ns1; d < 32u; d <<= 1) {
            const uint32_t t = (uint32_t)__shfl_up((int)pm, d, 64);
            if (hl >= d && lane < 32) pm = pm > t ? pm : t;
        }
        uint32_t before = (uint32_t)__shfl_up((int)pm, ns1, 64); // ... of the earlier clips of my class in this pass
        if (hl < ns1) before = 0u;
        uint32_t cprev = 0u;                                     // ... and of the passes before
#pragma unroll
        for (int q = 0; q < RB_MS; q++) cprev = (cls == (uint32_t)q) ? carry[q] : cprev;
        before = before > cprev ? before : cprev;
        const bool in_slot = spec && streams && emits && e_cnt != 0u && eg_f >= before;
        const bool copied = emits && !in_slot; // (an empty clip cannot happen: out_n >= 1 for an OK row)
        if (jb + RB_HMAX < (BRK ? n_items : nh)) { // another pass follows: what it must stay behind
#pragma unroll
            for (int q = 0; q < RB_MS; q++) {
                uint32_t v = (lane < 32 && cls == (uint32_t)q) ? pm : 0u;
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) {
                    const uint32_t o = (uint32_t)__shfl_xor((int)v, off, 64);
                    v = v > o ? v : o;
                }
                carry[q] = carry[q] > v ? carry[q] : rb_first(v);
            }
        }
        // (dead: the round-2 end-group patch read the record again through it.  Without the declaration the list kernel's register
        //  assignment moves -- two register pairs trade places --, so it stays until a change that is measured on the GPU anyway)
        [[maybe_unused]] const uint32_t *__restrict__ gsrc = rec_ops - head;
        RB_PHASE(2)
        const uint64_t my_off = (uint64_t)cls * slot_stride_ + slot_row0 + e_first; // out_ops index of my clip's first op
        // (the row index is formed from an opaque copy of the lane id: otherwise the compiler hoists the row addresses above
        //  the streaming loop and carries -- or spills -- them through it)
        uint32_t lane_late = (uint32_t)lane;
        asm volatile("" : "+v"(lane_late));
        const uint64_t my_row = (BRK ? brk_row0 + jb : h0 + jb) + lane_late;
        if (mine) {
            rb_hit_row *row = &p.rows[my_row];
            if (defer) {
                row->rec = r;
                row->win = win;
                row->flags = RB_HIT_GENERIC;
                const unsigned long long g = atomicAdd((unsigned long long *)&p.counters->n_generic, 1ull);
                p.gen_list[g] = (uint32_t)my_row;
            } else {
                rb_hit_row w;
                w.rec = r;
                w.win = win;
                w.status = (uint16_t)status;
                w.flags = (inside ? RB_HIT_INSIDE : 0) | ((desc_mode_ && status == RB_ST_OK) ? RB_HIT_DESCRIPTOR : 0);
                w.out_n = status == RB_ST_OK ? out_n : 0;
                w.t_st = o_tst;
                w.t_en = o_ten;
                w.q_st = o_qst;
                w.q_en = o_qen;
                w.nmatch = o_nm;
                w.aln_len = o_al;
                w.out_off = status == RB_ST_OK ? (desc_mode_ ? 4ull * my_row : (in_slot ? my_off : 0ull)) : 0; // (copied clips: rb_k_copy_clips fills it in)
                *row = w;
                if (desc_mode_ && status == RB_ST_OK) // which ops of the ORIGINAL cigar the clip keeps
                    *reinterpret_cast<uint4 *>(out_ops_ + 4ull * my_row) =
                        make_uint4(nr->first_op + a_op, out_n, inside ? 0u : rb_part(A.part), inside ? 0u : rb_part(B.part));
            }
        }
        RB_PHASE(3)
        // ---- the end ops, written by the lane that owns the clip: the speculative stores put the record's ops there as they are; the clip's first op keeps its tail, its last op
        //      its head.  Both words are made from what the resolution of the two boundaries left in registers (clipped length and op code:
        //      rb_bres.part) -- nothing is read again.  A clip that is the middle of ONE op holds B.U - A.U units of it.
        //      (diagnostics, dbg & 512: what the end ops cost -- their stores are left out) ----
        if (in_slot && !inside && !(dbg & (1 | 512))) {
            uint32_t *__restrict__ dst = out_ops_ + (uint64_t)cls * slot_stride_ + slot_row0; // coordinate 0
            if (e_cnt == 1u) {
                __builtin_nontemporal_store(((B.U - A.U) << 4) | (A.part >> 28), dst + e_first);
            } else {
                __builtin_nontemporal_store(rb_part_word(A.part), dst + e_first);
                __builtin_nontemporal_store(rb_part_word(B.part), dst + eg_last);
            }
        }
        // ---- clips without a place of their own: one list entry each, copied by rb_k_copy_clips ----
        {
            const unsigned long long cm = __ballot(copied);
            if (cm) {
                unsigned long long c0 = 0;
                if (lane == 0) c0 = atomicAdd(p.copy_count, (unsigned long long)__popcll(cm));
                c0 = rb_first64(c0);
                if (copied) {
                    const uint64_t at = c0 + (uint64_t)__popcll(cm & ((1ull << lane) - 1ull));
                    p.copy_list[at] = make_uint4((uint32_t)my_row, a_op, inside ? 0u : rb_part(A.part), inside ? 0u : rb_part(B.part));
                }
            }
        }
        RB_PHASE(4)
        } // (behind the stream)
    }
    if ((dbg & 256) && lane == 0) p.diag_stamps[wave] = (uint32_t)__builtin_amdgcn_s_memrealtime();
}
#undef p
