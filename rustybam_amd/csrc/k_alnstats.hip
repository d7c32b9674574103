// k_alnstats.hip -- what a stats line of an ALIGNMENT record (SAM / BAM) needs besides the record scan (gfx950, wave64):
//
//   rb_k_parse_md    replaces bamstats::parse_md_for_stats (bamstats.rs:48-79): the regex (\d+)|([A-Z])|(\^[A-Z]+) applied left to right
//                    over an MD:Z: value, restated as RUNS so that no byte depends on a state carried along the string:
//                      every maximal digit run adds its value;  every maximal run of A-Z whose preceding byte is '^' is one deletion
//                      event of that many bases;  every other A-Z byte is one mismatch;  every other byte is skipped.
//                    Sums wrap in u32.  A digit run of ten or more digits is left to the host (RB_MD_UNUSUAL), as rb_k_parse_cigars does.
//   rb_k_aln_stats   replaces the per-record body of bamstats::cigar_stats (bamstats.rs:129-142, :190-207): reference end, query span
//                    with rust-htslib's read_pos preconditions (rb_span.h, shared with the host), the strand flip, the MD refinement
//                    of M.  One lane per alignment.
//
// Shape of rb_k_parse_md: the idiom of k_hitstats.hip / k_rows_batch.hip.  A string is a ROW of 16 lanes, four strings to a wavefront,
// 16 bytes per lane and step (256 contiguous bytes per row and step); strings of more than RB_MD_ROW_MAX bytes are left out of the row
// form and walked afterwards by the whole wavefront (1 KiB per step).  A lane classifies its 16 bytes SWAR on the dwords into three
// 16-bit maps (digit, A-Z, '^'); everything about the letters is bit arithmetic on the maps:
//   - a run of A-Z that starts inside the lane is a deletion iff the map of '^' has the bit in front of it; an add of the start bits
//     to the map of A-Z carries through exactly the bits of those runs;
//   - the lane's LEADING letters continue whatever run reaches them: the nearest earlier lane that holds a byte that is no letter
//     (a ballot) says through one bit (a second ballot: "its last such byte is '^'") whether that run is a deletion; a register
//     carries the answer from one step to the next.  No lane looks at the lanes before it one by one.
// Only the VALUES of the digit runs take the bytes one after the other, inside the lane (acc = acc * 10 + digit, added and reset
// behind a run); a number that straddles two lanes is completed with the previous lane's unfinished digits (DPP row_shr:1 /
// wave_shr:1), which a register carries across steps too.
//
// Memory.  Only aligned 16-byte groups that hold at least one byte of a string are loaded; bytes of a group outside the string are
// replaced by spaces before anything looks at them.  Algorithmic bytes: the MD bytes once + 16 B per record (two offsets) read,
// 17 B per record written.  rb_k_aln_stats: 72 + 24 (+ 18 with MD) B per record read, a few ops at both ends of the CIGAR, 80 B written.
#include "rb_device.h"
#include "rb_launch.h"
#include "rb_ratio.h"
#include "rb_span.h"

#define RB_MD_ROW_STEP 256u   // bytes per step of a row of 16 lanes
#define RB_MD_WAVE_STEP 1024u // bytes per step of the whole wavefront (long strings)
// (the two below can be set from the command line: tools/mkvariant.sh --src k_alnstats.hip builds the shapes profiles/sam_stats_summary.md compares)
#ifndef RB_MD_ROW_MAX
#define RB_MD_ROW_MAX 2048u   // strings of more bytes than this take the wavefront form (0: every string does, one after the other); rows win up to 2048, a tie from 4096 on (profiles/sam_stats_summary.md)
#endif
#ifndef RB_MD_BATCH
#define RB_MD_BATCH 2         // steps whose loads are in flight together
#endif

__device__ __constant__ uint32_t rb_md_pow10[10] = {1u, 10u, 100u, 1000u, 10000u, 100000u, 1000000u, 10000000u, 100000000u, 1000000000u};

struct rb_md_sums {
    uint32_t m, mm, ic, ib; // per lane: digit-run values, mismatches, deletion events, deletion bases
    uint32_t unusual;       // a digit run of ten or more digits
};

// bit 7 of every byte of y (bytes below 0x80) that is >= c
__device__ __forceinline__ uint32_t rb_md_ge(uint32_t y, uint32_t c) { return (y + (0x80u - c) * 0x01010101u) & 0x80808080u; }
// bit 7 of each of the four bytes -> bits 0..3
__device__ __forceinline__ uint32_t rb_md_nib(uint32_t t) {
    t >>= 7;
    t |= t >> 7;
    t |= t >> 14;
    return t & 15u;
}

// The walk of one string text[b0 .. b1) by W lanes (16: a row, every row of the wavefront its own string; 64: the wavefront).  Every
// lane of the wavefront runs every step (the ballots and DPP moves need them all); take == false: the lanes see spaces only.
// Returns the group's unfinished number behind the last step (the string ended in digits at the very end of a step).
template <int W>
__device__ __forceinline__ uint32_t rb_md_walk(const uint8_t *text, const uint64_t b0, const uint64_t b1, const bool take, const int lane, rb_md_sums &a) {
    static_assert((W == 16 && 16 * W == RB_MD_ROW_STEP) || (W == 64 && 16 * W == RB_MD_WAVE_STEP), "a step is one 16-byte load per lane");
    const uint32_t gl = (uint32_t)lane & (uint32_t)(W - 1);
    const uint32_t gbase = (uint32_t)lane & ~(uint32_t)(W - 1);
    const uint64_t a0 = b0 & ~15ull; // aligned start: the bytes in front of b0 are masked
    const uint64_t n_steps64 = take ? (b1 - a0 + (16u * W - 1u)) / (16u * W) : 0ull;
    uint32_t w_steps_hi = (uint32_t)(n_steps64 >> 32), w_steps_lo = (uint32_t)n_steps64; // the wavefront's steps: the longest of its strings
    if (W == 16) {
#pragma unroll
        for (int off = 16; off < 64; off <<= 1) {
            const uint32_t oh = (uint32_t)__shfl_xor((int)w_steps_hi, off, 64), ol = (uint32_t)__shfl_xor((int)w_steps_lo, off, 64);
            const bool gt = oh > w_steps_hi || (oh == w_steps_hi && ol > w_steps_lo);
            w_steps_hi = gt ? oh : w_steps_hi, w_steps_lo = gt ? ol : w_steps_lo;
        }
    }
    const uint64_t w_steps = ((uint64_t)rb_first(w_steps_hi) << 32) | rb_first(w_steps_lo);
    uint32_t carry_val = 0, carry_nd = 0; // the unfinished number at the end of the group's last lane in the previous step
    uint32_t carry_c15 = 0;               // that lane's last byte is '^'
    uint32_t carry_del = 0;               // letters at the start of this step continue a deletion run (or stand behind a '^')
    for (uint64_t s0 = 0; s0 < w_steps; s0 += RB_MD_BATCH) {
        uint4 pf[RB_MD_BATCH];
#pragma unroll
        for (int s = 0; s < RB_MD_BATCH; s++) {
            const uint64_t la = a0 + (s0 + (uint64_t)s) * (16u * W) + gl * 16u;
            pf[s] = make_uint4(0x20202020u, 0x20202020u, 0x20202020u, 0x20202020u);
            if (take && la < b1) pf[s] = *reinterpret_cast<const uint4 *>(text + la); // (the text is readable to the next multiple of 16)
        }
#pragma unroll
        for (int s = 0; s < RB_MD_BATCH; s++) {
            if (s0 + (uint64_t)s >= w_steps) break; // (uniform over the wavefront)
            const uint64_t la = a0 + (s0 + (uint64_t)s) * (16u * W) + gl * 16u;
            uint32_t w[4] = {pf[s].x, pf[s].y, pf[s].z, pf[s].w};
            const bool loaded = take && la < b1;
            const uint32_t fv = loaded && b0 > la ? (uint32_t)(b0 - la) : 0u;                        // bytes [fv, ev) of the chunk belong
            const uint32_t ev = loaded ? (b1 - la < 16u ? (uint32_t)(b1 - la) : 16u) : 16u;          // to the string (fv <= 15)
            if (rb_ballot(fv != 0u || ev != 16u) != 0ull) { // first / last chunk of a string only: bytes outside it read as spaces
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int32_t lo = (int32_t)fv - 4 * j, hi = (int32_t)ev - 4 * j;
                    const uint32_t l2 = lo < 0 ? 0u : (lo > 4 ? 4u : (uint32_t)lo), h2 = hi < 0 ? 0u : (hi > 4 ? 4u : (uint32_t)hi);
                    const uint32_t m = h2 > l2 ? ((0xFFFFFFFFu << (8u * l2)) & (0xFFFFFFFFu >> (32u - 8u * h2))) : 0u; // (l2 <= 3, h2 >= 1 here)
                    w[j] = (w[j] & m) | (0x20202020u & ~m);
                }
            }
            // ---- the three maps: bit i = byte i of the chunk is a digit / A-Z / '^' ----
            uint32_t Dg = 0, Up = 0, Ca = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t x = w[j], y = x & 0x7F7F7F7Fu, low = ~x & 0x80808080u; // (a byte of 0x80 and above is none of the three)
                Dg |= rb_md_nib(rb_md_ge(y, '0') & ~rb_md_ge(y, ':') & low) << (4 * j);
                Up |= rb_md_nib(rb_md_ge(y, 'A') & ~rb_md_ge(y, '[') & low) << (4 * j);
                Ca |= rb_md_nib(rb_md_ge(y, '^') & ~rb_md_ge(y, '_') & low) << (4 * j);
            }
            // ---- digit runs ----
            const uint32_t nd_map = ~Dg & 0xFFFFu;                                        // bytes that are no digit
            const bool seen = nd_map != 0u;
            const uint32_t lead_nd = seen ? (uint32_t)__builtin_ctz(nd_map) : 16u;        // digits in front of the first of them
            const uint32_t trail_nd = seen ? (uint32_t)__builtin_clz(nd_map) - 16u : 16u; // digits behind the last of them
            uint32_t acc = 0, sum = 0;
#pragma unroll
            for (int i = 0; i < 16; i++) { // the values: a run that ends in the lane is added where it ends
                const uint32_t d = (w[i >> 2] >> (8 * (i & 3))) & 15u;
                const uint32_t k = (uint32_t)__builtin_amdgcn_sbfe((int)Dg, i, 1);
                sum += acc & ~k;
                acc = (acc * 10u + d) & k;
            }
            uint32_t in_val, in_nd, prev_c15;
            const uint32_t c15 = (Ca >> 15) & 1u;
            if (W == 16) {
                in_val = (uint32_t)__builtin_amdgcn_update_dpp((int)carry_val, (int)acc, RB_DPP_ROW_SHR(1), 0xf, 0xf, false);
                in_nd = (uint32_t)__builtin_amdgcn_update_dpp((int)carry_nd, (int)trail_nd, RB_DPP_ROW_SHR(1), 0xf, 0xf, false);
                prev_c15 = (uint32_t)__builtin_amdgcn_update_dpp((int)carry_c15, (int)c15, RB_DPP_ROW_SHR(1), 0xf, 0xf, false);
                carry_val = rb_row_last(acc), carry_nd = rb_row_last(trail_nd), carry_c15 = rb_row_last(c15);
            } else {
                in_val = rb_prev_lane(acc, carry_val), in_nd = rb_prev_lane(trail_nd, carry_nd), prev_c15 = rb_prev_lane(c15, carry_c15);
                carry_val = rb_readlane<uint32_t>(acc, 63), carry_nd = rb_readlane<uint32_t>(trail_nd, 63), carry_c15 = rb_readlane<uint32_t>(c15, 63);
            }
            // the lane's first run takes the digits that came in from the lane before (a lane of digits only: sixteen of them)
            if (seen) sum += in_val * rb_md_pow10[lead_nd < 10u ? lead_nd : 9u];
            a.m += sum;
            {
                uint32_t rr = Dg & (Dg >> 1);
                rr &= rr >> 2;
                rr &= rr >> 4; // eight in a row
                if (!seen || in_nd + lead_nd >= 10u || (rr & (Dg >> 8) & (Dg >> 9))) a.unusual = 1u;
            }
            // ---- letters ----
            const uint32_t nu = ~Up & 0xFFFFu;                                  // bytes that are no letter
            const bool has_nu = nu != 0u;
            const uint32_t last_nu = has_nu ? 31u - (uint32_t)__builtin_clz(nu) : 0u;
            const unsigned long long NU = rb_ballot(has_nu);                    // lanes that end every run that reaches them
            const unsigned long long LC = rb_ballot(has_nu && ((Ca >> last_nu) & 1u)); // ... whose last such byte is '^'
            const unsigned long long below = (NU >> gbase) & ((1ull << gl) - 1ull);     // such lanes of my group in front of me
            const uint32_t lead_del = below ? (uint32_t)(LC >> (gbase + 63u - (uint32_t)__builtin_clzll(below))) & 1u : carry_del;
            const unsigned long long grp = W == 16 ? (NU >> gbase) & 0xFFFFull : NU;
            if (grp) carry_del = (uint32_t)(LC >> (gbase + 63u - (uint32_t)__builtin_clzll(grp))) & 1u;
            const uint32_t lead_len = (uint32_t)__builtin_ctz(nu | 0x10000u);   // leading letters (0 .. 16)
            const uint32_t lead_mask = (1u << lead_len) - 1u;
            const uint32_t starts = Up & ~(Up << 1) & ~1u;                      // runs that start inside the lane
            const uint32_t dst = starts & (Ca << 1);                            // ... behind a '^'
            const uint32_t filled = ((Up + dst) ^ Up) & Up;                     // the bytes of those runs (the add carries through them)
            a.ib += (uint32_t)__builtin_popcount(filled) + (lead_del ? lead_len : 0u);
            a.ic += (uint32_t)__builtin_popcount(dst) + ((lead_len != 0u && prev_c15 != 0u) ? 1u : 0u);
            a.mm += (uint32_t)__builtin_popcount(Up & ~filled & ~lead_mask) + (lead_del ? 0u : lead_len);
        }
    }
    return carry_val;
}

template <int W>
__device__ __forceinline__ void rb_md_finish(const rb_md_sums &a, const uint32_t tail_val, const int lane, const bool write, uint32_t *out4, uint8_t *status) {
    const uint32_t gbase = (uint32_t)lane & ~(uint32_t)(W - 1);
    uint32_t m, mm, ic, ib;
    if (W == 16) m = rb_row_sum(a.m), mm = rb_row_sum(a.mm), ic = rb_row_sum(a.ic), ib = rb_row_sum(a.ib);
    else m = rb_wave_sum_u32(a.m), mm = rb_wave_sum_u32(a.mm), ic = rb_wave_sum_u32(a.ic), ib = rb_wave_sum_u32(a.ib);
    const unsigned long long un = rb_ballot(a.unusual != 0u);
    const bool unusual = (W == 16 ? (un >> gbase) & 0xFFFFull : un) != 0ull;
    if (!write) return;
    // (an unusual string's counts are not the device's to give: zero, and the status says so)
    *reinterpret_cast<uint4 *>(out4) = unusual ? make_uint4(0u, 0u, 0u, 0u) : make_uint4(m + tail_val, mm, ic, ib);
    *status = (uint8_t)(unusual ? RB_MD_UNUSUAL : RB_MD_OK);
}

__global__ __launch_bounds__(256) void rb_k_parse_md(rb_md_params p) {
    const int lane = rb_lane();
    const uint32_t gl = (uint32_t)lane & 15u;
    const uint64_t k0 = ((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6)) * 4u; // the wavefront's first string
    const uint64_t k = k0 + ((uint32_t)lane >> 4);
    const bool live = k < p.n;
    uint64_t b0 = 0, b1 = 0;
    if (live) b0 = p.md_off[k], b1 = p.md_end[k];
    if (b1 < b0) b1 = b0; // (an extent that ends before it starts is the empty string)
    const bool is_long = live && b1 - b0 > (uint64_t)RB_MD_ROW_MAX;
    const bool take = live && !is_long;
    rb_md_sums a = {0u, 0u, 0u, 0u, 0u};
    const uint32_t tail = rb_md_walk<16>(p.text, b0, b1, take && b1 > b0, lane, a); // (an empty string reads nothing, wherever its offset points)
    rb_md_finish<16>(a, tail, lane, take && gl == 0u, p.out + 4u * k, p.status + k);
    // ---- the long strings of these four rows, one after the other, by the whole wavefront ----
    unsigned long long todo = rb_ballot(is_long && gl == 0u);
    while (todo) {
        const uint32_t b = (uint32_t)__builtin_ctzll(todo);
        todo &= todo - 1ull;
        const uint64_t kk = k0 + (b >> 4);
        const uint64_t l0 = rb_first64(p.md_off[kk]), l1 = rb_first64(p.md_end[kk]);
        rb_md_sums al = {0u, 0u, 0u, 0u, 0u};
        const uint32_t tl = rb_md_walk<64>(p.text, l0, l1, true, lane, al);
        rb_md_finish<64>(al, tl, lane, lane == 0, p.out + 4u * kk, p.status + kk);
    }
}

// ---- the span and the MD refinement: one lane per alignment ----
// The ends of the CIGAR say everything (rb_span.h) but one thing: that no hard clip stands between the first op of the read and the op
// that holds the last reference base.  A lane looks at those ops itself when they are few; the longer stretches of a wavefront's
// records are looked at afterwards by all 64 lanes together, 64 ops per step.
#define RB_ALN_LANE_SCAN 32u // ops between the two ends that a lane checks alone
__global__ __launch_bounds__(256) void rb_k_aln_stats(rb_alnstats_params p) {
    const int lane = rb_lane();
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const bool live = r < p.n;
    uint64_t o0 = 0, nc = 0;
    rb_reduce_row red;
    red.t_bases = red.q_bases = 0;
    if (live) o0 = p.op_off[r], nc = p.op_off[r + 1] - o0, red = p.reduce_rows[r];
    const uint32_t *cg = p.ops + o0;
    rb_span_ends sp;
    sp.status = RB_ALN_PANIC_NONE, sp.j = sp.e = 0;
    if (live) sp = rb_span_ends_of(cg, nc, red.t_bases);
    const bool scan = (sp.status == RB_ALN_OK || sp.status == RB_ALN_PANIC_NONE) && sp.e > sp.j;
    const uint64_t n_scan = scan ? sp.e - sp.j : 0ull;
    bool inner = false;
    if (n_scan != 0 && n_scan <= RB_ALN_LANE_SCAN) inner = rb_span_inner_clip(cg, sp.j, sp.e);
    unsigned long long todo = rb_ballot(n_scan > RB_ALN_LANE_SCAN);
    while (todo) { // (uniform: every lane of the wavefront is here)
        const int b = __builtin_ctzll(todo);
        todo &= todo - 1ull;
        const uint64_t first = rb_readlane<uint64_t>(o0 + sp.j, b), cnt = rb_readlane<uint64_t>(n_scan, b);
        bool hit = false;
        for (uint64_t i = (uint64_t)lane; i < cnt; i += 64u) hit = hit || rb_span_clip_like(p.ops[first + i] & 15u);
        const bool any = rb_ballot(hit) != 0ull;
        if (lane == b) inner = any;
    }
    if (!live) return;
    rb_aln_row w;
    w.r_en = w.q_st = w.q_en = w.q_len = 0;
    w.equal = w.diff = w.ins = w.del = w.matches = w.ins_events = w.del_events = 0u;
    w.id_by_all = w.id_by_events = w.id_by_matches = 0.0f;
    w.status = RB_ALN_OK, w.flags = 0u;
    const rb_aln_row zero = w; // a row whose status is not RB_ALN_OK carries nothing else
    uint32_t st = rb_span_status(sp, inner);
    if (st == RB_ALN_OK) {
        const int64_t qpos = (int64_t)red.q_bases - sp.q_after - 1; // S and I count as read bases, H does not
        w.r_en = p.pos[r] + (int64_t)red.t_bases;                   // CigarStringView::end_pos
        w.q_st = sp.lead_h + sp.lead_s;
        w.q_en = sp.lead_h + 1 + qpos;
        w.q_len = sp.lead_h + (int64_t)p.l_seq[r] + sp.trail_h;
        if (p.flag[r] & 16u) { // bamstats.rs:203-207
            const int64_t t = w.q_st;
            w.q_st = w.q_len - w.q_en;
            w.q_en = w.q_len - t;
        }
        w.equal = red.equal, w.diff = red.diff, w.ins = red.ins, w.del = red.del, w.matches = red.matches;
        w.ins_events = red.ins_events, w.del_events = red.del_events;
        w.id_by_all = red.id_by_all, w.id_by_events = red.id_by_events, w.id_by_matches = red.id_by_matches;
        const bool has_md = p.has_md && p.has_md[r] != 0;
        if (w.equal == 0u && w.matches > 0u && has_md) { // bamstats.rs:129-142
            const uint32_t mst = p.md_status ? p.md_status[r] : 0u;
            const uint32_t m = p.md[4u * r], mm = p.md[4u * r + 1u];
            if (mst != RB_MD_OK) st = RB_ALN_MD_STATUS | mst;
            else if (m + mm != w.diff) st = RB_ALN_PANIC_MD_ASSERT;
            else {
                w.equal = m, w.diff = mm;
                rb_identity_ratios(w);
            }
        } else if (w.matches > 0u && !has_md) {
            w.flags |= RB_ALN_WARN_M; // bamstats.rs:145-153
        }
    }
    if (st != RB_ALN_OK) {
        w = zero;
        w.status = st;
    }
    p.rows[r] = w;
}

extern "C" hipError_t rb_launch_parse_md(const rb_md_params *p, hipStream_t stream) {
    if (p->n == 0) return hipSuccess;
    hipLaunchKernelGGL(rb_k_parse_md, dim3((unsigned)((p->n + 15) / 16)), dim3(256), 0, stream, *p);
    return hipGetLastError();
}
extern "C" hipError_t rb_launch_aln_stats(const rb_alnstats_params *p, hipStream_t stream) {
    if (p->n == 0) return hipSuccess;
    hipLaunchKernelGGL(rb_k_aln_stats, dim3((unsigned)((p->n + 255) / 256)), dim3(256), 0, stream, *p);
    return hipGetLastError();
}
extern "C" uint32_t rb_md_row_step(void) { return RB_MD_ROW_STEP; }
extern "C" uint32_t rb_md_wave_step(void) { return RB_MD_WAVE_STEP; }
extern "C" uint32_t rb_md_row_max(void) { return RB_MD_ROW_MAX; }
