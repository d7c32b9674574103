// k_hitstats.hip -- stats of every hit row's clip where it lies (gfx950, wave64): rb_dev_stats_rows.
//
// What `rb liftover ... | rb stats --paf` computes per printed record -- bamstats::stats_from_paf (bamstats.rs:91-154) and the
// check_integrity of the Paf::from_file that reads it back (paf.rs:825-857) -- from the ops of the clip the clip kernel left in HBM:
// plain ops in out_ops, or a 4-word descriptor into the batch (RB_LIFT_DESCRIPTORS), both in one call.  One rb_reduce_row per hit row.
//
// Shape.  Clips run from one op (break-paf pieces, window edges) to whole records of 80k ops (RB_HIT_INSIDE rows); the headline batch
// averages 480 per hit.  A hit is a ROW of 16 lanes (rb_device.h), four hits to a wavefront, exactly as the record scan's row form
// (k_records.hip, rb_k_scan_rows): a lane takes the aligned 16-byte groups gl, gl + 16, ... of its clip, so a row's load is 256
// contiguous bytes and a row's step RB_HS_ROW_STEP = 64 ops; RB_HS_BATCH steps are in flight together; the per-class sums go through
// the same LDS counters (one 64-bit counter per lane and op code: length in the low 40 bits, op count above) and are reduced with DPP
// sums inside the row, so one instruction stream finishes four hits and four lanes write their rows side by side.
// A clip of more than RB_HS_ROW_MAX ops would hold the other three rows of its wavefront up for as many steps: the row form leaves it
// out, and the SAME wavefront walks it afterwards with all 64 lanes (a step of RB_HS_WAVE_STEP = 256 ops, 1 KiB per load instruction).
// No list, no atomics on global memory, no second launch and no second read of the rows: which wavefront walks a long clip is fixed by
// the row's index, so two calls write the same bytes.
//
// Memory.  Only aligned 16-byte groups that hold at least one word of a clip (or of a descriptor) are loaded: the first group is the
// one the clip's first word lies in, and a load past the clip's last group re-reads that last group and is masked.
// Roofline: 64 B per row read, 72 B per row written, 4 B per clip op (+ 16 B per descriptor).
#include "rb_device.h"
#include "rb_launch.h"
#include "rb_ratio.h"
#include <type_traits>

#define RB_HS_ROW_STEP 64u   // ops per step of a row of 16 lanes (4 per lane)
#define RB_HS_WAVE_STEP 256u // ops per step of the whole wavefront (long clips)
// (the two below can be set from the command line: tools/mkvariant.sh --src k_hitstats.hip builds the shapes profiles/hitstats_summary.md compares)
#ifndef RB_HS_ROW_MAX
#define RB_HS_ROW_MAX 4096u  // clips of more ops than this take the wavefront form (0: every clip does, one after the other)
#endif
#ifndef RB_HS_BATCH
#define RB_HS_BATCH 4        // steps whose loads are in flight together (2 and 8 measured slower or equal: profiles/hitstats_summary.md)
#endif
#define RB_HS_LEN_BITS 40

struct rb_hs_clip {
    const uint32_t *gsrc; // the aligned group that holds the clip's first word
    uint32_t head;        // words of that group in front of the clip (0 .. 3)
    uint32_t n;           // words of the clip
    uint32_t fl, ll;      // descriptor rows: != 0 replaces the length of the first / last op
};

// where the clip of an RB_ST_OK row lies (rb_k_digest_rows and the host's rows_to_text follow the same rules)
__device__ __forceinline__ rb_hs_clip rb_hs_locate(const rb_hitstats_params &p, const rb_hit_row &h) {
    rb_hs_clip c;
    const uint32_t *src = p.out_ops + h.out_off;
    c.n = h.out_n;
    c.fl = c.ll = 0u;
    if (h.flags & RB_HIT_DESCRIPTOR) { // {first kept op in the record's original cigar, op count, first length, last length}
        const uint32_t first = src[0];
        c.n = src[1];
        if (!(h.flags & RB_HIT_INSIDE)) c.fl = src[2], c.ll = src[3];
        src = p.ops + p.op_off[h.rec] + first; // (op_off as a table of starts: a batch in RB_LIFT_OP_STARTS form works)
    }
    c.head = (uint32_t)(((uintptr_t)src >> 2) & 3u);
    c.gsrc = src - c.head;
    return c;
}

// The walk of one clip by W lanes (16: a row, every row of the wavefront its own clip; 64: the wavefront): every lane adds the ops of
// its groups to its own LDS counters hist[code][lane].  take == false: the lanes sit the walk out (row form only).
template <int W>
__device__ __forceinline__ void rb_hs_walk(const rb_hs_clip &c, const bool take, unsigned long long (*hist)[64], const int lane) {
    static_assert((W == 16 && 4 * W == RB_HS_ROW_STEP) || (W == 64 && 4 * W == RB_HS_WAVE_STEP), "a step is one 16-byte load per lane");
    const uint32_t gl = (uint32_t)lane & (uint32_t)(W - 1);
    const uint64_t span = (uint64_t)c.head + c.n;
    const uint32_t n = c.n;
    const bool one_both = n == 1u && c.fl && c.ll;
    const uint32_t n_steps = take ? (uint32_t)((span + (4u * W - 1u)) / (4u * W)) : 0u;
    const uint64_t last_off = take && n ? ((span - 1u) & ~3ull) : 0ull;
    uint32_t w_steps = n_steps; // the wavefront's steps: the longest of its clips
    if (W == 16) {
#pragma unroll
        for (int off = 16; off < 64; off <<= 1) {
            const uint32_t o = (uint32_t)__shfl_xor((int)w_steps, off, 64);
            w_steps = w_steps > o ? w_steps : o;
        }
    }
    w_steps = rb_first(w_steps);
    uint32_t carry_w = 0xFu; // last word of the previous step (code 15 owns no continuation word)
    for (uint32_t b0 = 0; b0 < w_steps; b0 += RB_HS_BATCH) {
        uint4 pf[RB_HS_BATCH];
#pragma unroll
        for (int s = 0; s < RB_HS_BATCH; s++) {
            uint64_t off = (uint64_t)(b0 + (uint32_t)s) * (4u * W) + gl * 4u;
            off = off < last_off ? off : last_off; // (past the clip's end: its last group again; masked below)
            pf[s] = (take && n) ? *reinterpret_cast<const uint4 *>(c.gsrc + off) : make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (int s = 0; s < RB_HS_BATCH; s++) {
            const uint32_t st = b0 + (uint32_t)s;
            if (st < n_steps) { // (uniform over the W lanes: a row whose clip has ended sits the step out)
                const uint32_t raw[4] = {pf[s].x, pf[s].y, pf[s].z, pf[s].w};
                const uint32_t idx0 = st * (4u * W) + gl * 4u - c.head; // index of raw[0] in the clip (wraps below 0 in front of it)
                // a step that is some clip's first or last one masks the words of the neighbours and patches the descriptor's end lengths
                const bool my_edge = st == 0u || st + 1u == n_steps;
                const bool any_edge = W == 16 ? rb_ballot(my_edge) != 0ull : my_edge;
                auto step = [&](auto edge_c) {
                    constexpr bool edge = decltype(edge_c)::value;
                    uint32_t mylast = raw[3];
                    if (edge && idx0 + 3u >= n) mylast = 0xFu;
                    uint32_t prevw;
                    if (W == 16) {
                        prevw = (uint32_t)__builtin_amdgcn_update_dpp((int)carry_w, (int)mylast, RB_DPP_ROW_SHR(1), 0xf, 0xf, false);
                        carry_w = rb_row_last(mylast);
                    } else {
                        prevw = rb_prev_lane(mylast, carry_w);
                        carry_w = rb_readlane<uint32_t>(mylast, 63);
                    }
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const uint32_t idx = idx0 + (uint32_t)q;
                        const bool ok = !edge || idx < n;
                        const uint32_t w = raw[q], opc = w & 15u;
                        uint32_t len = w >> 4;
                        if (edge) {
                            if (one_both) len = c.fl + c.ll - len; // (idx == 0 is the only word there is)
                            else {
                                if (idx == 0u && c.fl) len = c.fl;
                                if (idx == n - 1u && c.ll) len = c.ll;
                            }
                        }
                        if (ok) {
                            if (opc <= 8u) {
                                __hip_atomic_fetch_add(&hist[opc][lane], (unsigned long long)len | (1ull << RB_HS_LEN_BITS), __ATOMIC_RELAXED,
                                                       __HIP_MEMORY_SCOPE_WORKGROUP);
                            } else {
                                // as rb_k_scan_records: a continuation word adds payload << 28 to its owner's class and is no event; any other word
                                // of a code above 8 consumes nothing, its length counts in the unit total alone (kept with P's)
                                const bool cont = opc == RB_OP_CONT && (prevw & 15u) <= 8u;
                                __hip_atomic_fetch_add(&hist[cont ? (prevw & 15u) : (uint32_t)RB_OP_P][lane],
                                                       cont ? (unsigned long long)(len & 15u) << RB_LEN_BITS_WORD : (unsigned long long)len, __ATOMIC_RELAXED,
                                                       __HIP_MEMORY_SCOPE_WORKGROUP);
                            }
                        }
                        prevw = ok ? w : 0xFu;
                    }
                };
                if (any_edge) step(std::true_type{});
                else step(std::false_type{});
            }
        }
    }
}

// the sums of a lane's group (W lanes) from the LDS counters, and the stats row from them (one lane writes)
template <int W>
__device__ __forceinline__ uint32_t rb_hs_sum(uint32_t v) {
    return W == 16 ? rb_row_sum(v) : rb_wave_sum_u32(v);
}
template <int W>
__device__ __forceinline__ void rb_hs_finish(unsigned long long (*hist)[64], const int lane, const bool write, const rb_hit_row &h, rb_reduce_row *dst) {
    uint64_t L[9];
    auto sum40 = [&](unsigned long long v) -> uint64_t { // a lane's length sum stays below 2^40: two 20-bit pieces
        const uint32_t s_lo = rb_hs_sum<W>((uint32_t)v & 0xFFFFFu), s_hi = rb_hs_sum<W>((uint32_t)(v >> 20) & 0xFFFFFu);
        return (uint64_t)s_lo + ((uint64_t)s_hi << 20);
    };
#pragma unroll
    for (int t = 0; t < 9; t++) L[t] = sum40(hist[t][lane]);
    const uint32_t ins_events = rb_hs_sum<W>((uint32_t)(hist[RB_OP_I][lane] >> RB_HS_LEN_BITS));
    const uint32_t del_events = rb_hs_sum<W>((uint32_t)(hist[RB_OP_D][lane] >> RB_HS_LEN_BITS));
    if (!write) return;
    // as rb_scan_finish (k_records.hip) writes the reduce row of a record with these ops and the hit row's coordinates
    const uint64_t R = L[RB_OP_M] + L[RB_OP_D] + L[RB_OP_N] + L[RB_OP_EQ] + L[RB_OP_X];
    const uint64_t Q = L[RB_OP_M] + L[RB_OP_I] + L[RB_OP_S] + L[RB_OP_EQ] + L[RB_OP_X];
    const uint64_t M = L[RB_OP_M] + L[RB_OP_EQ] + L[RB_OP_X];
    uint64_t U = 0;
#pragma unroll
    for (int t = 0; t < 9; t++) U += L[t];
    rb_reduce_row w;
    w.t_bases = R;
    w.q_bases = Q;
    w.nmatch = (uint32_t)M;
    w.aln_len = (uint32_t)U;
    w.equal = (uint32_t)L[RB_OP_EQ]; // bamstats.rs:107-127, u32 counters
    w.diff = (uint32_t)(L[RB_OP_X] + L[RB_OP_M]);
    w.ins = (uint32_t)L[RB_OP_I];
    w.del = (uint32_t)L[RB_OP_D];
    w.matches = (uint32_t)L[RB_OP_M];
    w.ins_events = ins_events;
    w.del_events = del_events;
    rb_identity_ratios(w); // bamstats.rs:138-142
    uint32_t st = RB_ST_OK;
    if (U > 0xFFFFFFFFull)
        st = RB_ST_PANIC_OVERFLOW;
    else if (h.t_en < h.t_st || h.t_en - h.t_st != R)
        st = RB_ST_PANIC_INTEGRITY_T;
    else if (h.q_en < h.q_st || h.q_en - h.q_st != Q)
        st = RB_ST_PANIC_INTEGRITY_Q;
    w.status = st;
    w.flags = L[RB_OP_M] != 0 ? (uint32_t)RB_F_HAS_M : 0u;
    *dst = w;
}

__global__ __launch_bounds__(256) void rb_k_hitstats(rb_hitstats_params p) {
    __shared__ unsigned long long hist_all[4][9][64];
    const int lane = rb_lane();
    const uint32_t gl = (uint32_t)lane & 15u;
    unsigned long long(*hist)[64] = hist_all[threadIdx.x >> 6];
    const uint64_t k0 = ((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6)) * 4u; // the wavefront's first row
    const uint64_t k = k0 + ((uint32_t)lane >> 4);
    const bool live = k < p.n_rows;
    rb_hit_row h;
    h.status = 0xFFFFu, h.flags = 0, h.out_n = 0, h.out_off = 0, h.rec = 0;
    h.t_st = h.t_en = h.q_st = h.q_en = 0;
    if (live) h = p.rows[k];
    const bool ok = live && h.status == RB_ST_OK;
    rb_hs_clip c;
    c.gsrc = p.out_ops, c.head = 0u, c.n = 0u, c.fl = c.ll = 0u;
    if (ok) c = rb_hs_locate(p, h);
    const bool is_long = ok && c.n > RB_HS_ROW_MAX;
    const bool take = ok && !is_long;
#pragma unroll
    for (int t = 0; t < 9; t++) hist[t][lane] = 0ull;
    rb_hs_walk<16>(c, take, hist, lane);
    rb_hs_finish<16>(hist, lane, take && gl == 0u, h, p.stats + k);
    if (live && !ok && gl == 0u) { // the reference dropped the pair or panicked: nothing to count
        rb_reduce_row w;
        w.t_bases = w.q_bases = 0;
        w.nmatch = w.aln_len = w.equal = w.diff = w.ins = w.del = w.matches = w.ins_events = w.del_events = 0;
        w.id_by_all = w.id_by_events = w.id_by_matches = 0.0f;
        w.status = h.status;
        w.flags = 0;
        p.stats[k] = w;
    }
    // ---- the long clips of these four rows, one after the other, by the whole wavefront ----
    unsigned long long todo = rb_ballot(is_long && gl == 0u);
    while (todo) {
        const uint32_t b = (uint32_t)__builtin_ctzll(todo);
        todo &= todo - 1ull;
        const uint64_t kk = k0 + (b >> 4);
        const rb_hit_row hl = p.rows[kk];
        const rb_hs_clip cl = rb_hs_locate(p, hl);
#pragma unroll
        for (int t = 0; t < 9; t++) hist[t][lane] = 0ull;
        rb_hs_walk<64>(cl, true, hist, lane);
        rb_hs_finish<64>(hist, lane, lane == 0, hl, p.stats + kk);
    }
}

extern "C" hipError_t rb_launch_hitstats(const rb_hitstats_params *p, hipStream_t stream) {
    if (p->n_rows == 0) return hipSuccess;
    hipLaunchKernelGGL(rb_k_hitstats, dim3((unsigned)((p->n_rows + 15) / 16)), dim3(256), 0, stream, *p);
    return hipGetLastError();
}
