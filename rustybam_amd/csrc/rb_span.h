// rb_span.h -- the query span of an alignment record, stated once for the device (k_alnstats.hip) and the host (host/rb_host.cpp).
//
// bamstats.rs:190-207 asks rust-htslib for read_pos(end_pos - 1): the position in the read of the LAST reference base, and unwraps it
// twice.  CigarStringView::read_pos (rust-htslib 0.44.1) walks the ops from the left; restated from both ends of the CIGAR:
//   1. from the left, up to the first op that describes read sequence (M I S = X): a D / N there is an Err, an H that is neither the
//      first nor the last op is an Err, and a CIGAR of H / P alone is None;                                    j = that first op
//   2. the last reference base lies in the last op of M D N = X that has a length;                              e = that op
//      (no such op, t_bases == 0: None)
//   3. on its way from j to e the walk must not meet an H (or a code that is no op): Err;
//   4. e is a D / N: the base is not in the read, None;  else the position is the read bases of the whole CIGAR minus those behind e,
//      minus one.
// Each Err / None is the reference's panic; which of them comes first is the order of the walk: 1, 3, then 2 / 4.
// Step 3 is the only one that looks at ops between the two ends; the callers run it (rb_span_inner_clip here, or the wavefront in
// k_alnstats.hip for long CIGARs).  Packed words as everywhere (len << 4 | op); a continuation word counts as a code that is no op.
#pragma once
#include <stdint.h>

#include "../../include/rustybam_amd.h"

#if defined(__HIPCC__)
#define RB_SPAN_FN __host__ __device__ inline
#else
#define RB_SPAN_FN inline
#endif

struct rb_span_ends {
    uint32_t status;                 // RB_ALN_OK, or the panic of steps 1 / 2 / 4 (step 3 is the caller's)
    uint64_t j, e;                   // steps 1 and 2 (valid when status is RB_ALN_OK or step 4's RB_ALN_PANIC_NONE)
    int64_t lead_h, lead_s, trail_h; // leading H, leading S (also behind an H), trailing H
    int64_t q_after;                 // read bases behind e
};

RB_SPAN_FN bool rb_span_clip_like(uint32_t o) { return o == RB_OP_H || o > 8u; }

RB_SPAN_FN rb_span_ends rb_span_ends_of(const uint32_t *cg, uint64_t nc, uint64_t t_bases) {
    rb_span_ends s;
    s.status = RB_ALN_OK, s.j = 0, s.e = 0, s.q_after = 0;
    s.lead_h = (nc && (cg[0] & 15u) == RB_OP_H) ? (int64_t)(cg[0] >> 4) : 0;
    s.lead_s = 0;
    if (nc && (cg[0] & 15u) == RB_OP_S) s.lead_s = (int64_t)(cg[0] >> 4);
    else if (nc > 1 && (cg[0] & 15u) == RB_OP_H && (cg[1] & 15u) == RB_OP_S) s.lead_s = (int64_t)(cg[1] >> 4);
    s.trail_h = (nc && (cg[nc - 1] & 15u) == RB_OP_H) ? (int64_t)(cg[nc - 1] >> 4) : 0;
    // 1.
    uint64_t j = 0;
    for (;; j++) {
        if (j == nc) { // (also the empty CIGAR)
            s.status = RB_ALN_PANIC_NONE;
            return s;
        }
        const uint32_t o = cg[j] & 15u;
        if (o == RB_OP_D || o == RB_OP_N) {
            s.status = RB_ALN_PANIC_DEL_FIRST;
            return s;
        }
        if (rb_span_clip_like(o) && j > 0 && j + 1 < nc) {
            s.status = RB_ALN_PANIC_HARDCLIP;
            return s;
        }
        if (!rb_span_clip_like(o) && o != RB_OP_P) break; // M I S = X
    }
    s.j = j;
    // 2.
    if (t_bases == 0) {
        s.status = RB_ALN_PANIC_NONE;
        return s;
    }
    uint64_t k = nc;
    for (; k > j; k--) {
        const uint32_t o = cg[k - 1] & 15u, l = cg[k - 1] >> 4;
        const bool ref = o == RB_OP_M || o == RB_OP_D || o == RB_OP_N || o == RB_OP_EQ || o == RB_OP_X;
        if (ref && l) break;
        if (o == RB_OP_M || o == RB_OP_I || o == RB_OP_S || o == RB_OP_EQ || o == RB_OP_X) s.q_after += (int64_t)l;
    }
    if (k == j) { // (t_bases disagrees with the ops)
        s.status = RB_ALN_PANIC_NONE;
        return s;
    }
    s.e = k - 1;
    // 4.
    const uint32_t oe = cg[s.e] & 15u;
    if (oe == RB_OP_D || oe == RB_OP_N) s.status = RB_ALN_PANIC_NONE;
    return s;
}

// 3. for the ops [j, e), one after the other
RB_SPAN_FN bool rb_span_inner_clip(const uint32_t *cg, uint64_t j, uint64_t e) {
    bool hit = false;
    for (uint64_t k = j; k < e; k++) hit = hit || rb_span_clip_like(cg[k] & 15u);
    return hit;
}
// the status of the record from the two: the walk meets an inner clip before it learns that e is a D / N
RB_SPAN_FN uint32_t rb_span_status(const rb_span_ends &s, bool inner_clip) {
    if (s.status != RB_ALN_OK && !(s.status == RB_ALN_PANIC_NONE && s.e > s.j)) return s.status; // steps 1, 2
    return inner_clip ? (uint32_t)RB_ALN_PANIC_HARDCLIP : s.status;
}
