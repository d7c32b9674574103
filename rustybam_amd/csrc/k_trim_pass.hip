// k_trim_pass.hip -- trim-paf around the pair step (k_trim.hip, k_trim4.hip), for gfx950: which pairs a pass cuts (rb_k_trim_select_rows,
// rb_k_trim_select, rb_k_trim_place), the worst status of its rows (rb_k_trim_check), and between two passes the clipped records made the
// batch's current ones (rb_k_apply_pairs) and gathered into a dense batch again (rb_k_gather_records).
#include "rb_device.h"
#include "rb_launch.h"

// ------------------------------------------------------------------------------------------------
// between two passes of trim-paf: the clipped records of a pass become the batch's current records (include/rustybam_amd.h,
// rb_dev_apply_pairs), and the current records gathered into a dense batch again (rb_dev_gather_records)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rb_k_apply_pairs(rb_apply_params p) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t k = t >> 1;
    const int s = (int)(t & 1);
    if (k >= p.n_pairs) return;
    const rb_pair_row *row = &p.rows[k];
    if (row->status != RB_ST_OK) return;
    const uint32_t rec = s ? p.right[k] : p.left[k];
    rb_norm_row n = p.norm[rec];
    n.t_st = row->t_st[s], n.t_en = row->t_en[s], n.q_st = row->q_st[s], n.q_en = row->q_en[s];
    n.first_op = 0, n.n_ops = row->out_n[s];
    n.lead_ops = n.trail_ops = 0; // (a clip starts and ends on a match op: remove_trailing_indels finds nothing, paf.rs:218-220)
    n.nmatch = row->nmatch[s], n.aln_len = row->aln_len[s];
    p.norm[rec] = n;
    p.op_off[rec] = row->out_off[s];
}
extern "C" hipError_t rb_launch_apply_pairs(const rb_apply_params *p, hipStream_t stream) {
    if (p->n_pairs == 0) return hipSuccess;
    hipLaunchKernelGGL(rb_k_apply_pairs, dim3((unsigned)((2 * p->n_pairs + 255) / 256)), dim3(256), 0, stream, *p);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void rb_k_gather_records(rb_gather_params p) {
    if (!p.fill) { // the kept length of every record
        const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
        if (r < p.n_rec) p.new_off[r] = p.norm[r].status == RB_ST_OK ? p.norm[r].n_ops : 0u;
        return;
    }
    const uint64_t r = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (r >= p.n_rec) return;
    const uint64_t n = p.new_off[r + 1] - p.new_off[r];
    const uint32_t *src = p.ops + p.op_off[r] + p.norm[r].first_op;
    uint32_t *dst = p.new_ops + p.new_off[r];
    for (uint64_t j = rb_lane(); j < n; j += 64) dst[j] = src[j];
}
extern "C" hipError_t rb_launch_gather_records(const rb_gather_params *p, hipStream_t stream) {
    if (p->n_rec == 0) return hipSuccess;
    if (!p->fill) hipLaunchKernelGGL(rb_k_gather_records, dim3((unsigned)((p->n_rec + 255) / 256)), dim3(256), 0, stream, *p);
    else hipLaunchKernelGGL(rb_k_gather_records, dim3((unsigned)((p->n_rec + 3) / 4)), dim3(256), 0, stream, *p);
    return hipGetLastError();
}


// ------------------------------------------------------------------------------------------------
// trim-paf: the pass driver's heavy half on the device (round 3).  Paf::overlapping_paf_recs (paf.rs:223-284) scans, per query
// name, all pairs of records for overlaps on the query (bed::get_overlap, bed.rs:74-85), flags contained records (:244-249),
// sorts ALL pairs by overlap (descending, stable) and then takes the first pair of every query name (:264-284).  Per query group
// that is: the pair with the LARGEST overlap, among equals the FIRST in scan order (i ascending, then j) -- a segmented arg-max, no
// global sort.  Groups are independent, so one pass = one launch: rb_k_trim_select_rows (groups of up to 16 records, a group per row of
// 16 lanes) and rb_k_trim_select (the larger groups: a thread per group; groups of more than RB_TS_BIG records by the whole wave, one
// after the other), an exclusive scan that gives the chosen pairs dense slots and their
// places in the ops arena, rb_k_trim_place.  The host keeps only the recursion loop (:286-288) and reads 64 bytes per pass.
// ------------------------------------------------------------------------------------------------
#define RB_TS_BIG 48u

struct rb_tsel_best {
    uint64_t ov;  // overlap (0: none yet)
    uint64_t ord; // scan order i * m + j of the pair that holds it
    uint32_t l, r;
};
__device__ __forceinline__ void rb_tsel_pair(const rb_tsel_params &p, uint32_t ri, uint32_t rj, uint64_t ord, rb_tsel_best &b, uint64_t &n_pairs) {
    const rb_norm_row *a = &p.norm[ri], *c = &p.norm[rj];
    const uint64_t st1 = a->q_st, en1 = a->q_en, st2 = c->q_st, en2 = c->q_en;
    const uint64_t mn = en1 < en2 ? en1 : en2, mx = st1 > st2 ? st1 : st2;
    if (mn <= mx) return;                       // bed.rs:74-85: no overlap
    const uint64_t ov = mn - mx;
    if (ov == en2 - st2) { p.contained[rj] = 1; return; } // paf.rs:244-249
    if (ov == en1 - st1) { p.contained[ri] = 1; return; }
    n_pairs++;
    if (ov > b.ov || (ov == b.ov && ord < b.ord)) {
        b.ov = ov, b.ord = ord;
        if (st1 <= st2) b.l = ri, b.r = rj; // the smaller q_st is "left" (:252-256)
        else b.l = rj, b.r = ri;
    }
}
// (groups of up to 16 records belong to rb_k_trim_select_rows, further down: this kernel leaves them alone)
__global__ __launch_bounds__(256) void rb_k_trim_select(rb_tsel_params p) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = rb_lane();
    const uint64_t gg0 = g < p.n_groups ? p.grp_off[g] : 0, gm = g < p.n_groups ? p.grp_off[g + 1] - gg0 : 0;
    const bool live = g < p.n_groups && gm > 16u;
    const uint64_t g0 = live ? gg0 : 0, m = live ? gm : 0;
    for (uint64_t k = 0; k < m && m <= RB_TS_BIG; k++) p.contained[p.order[g0 + k]] = 0;
    rb_tsel_best b = {0, 0, 0, 0};
    uint64_t n_pairs = 0;
    if (live && m <= RB_TS_BIG) {
        for (uint64_t i = 0; i + 1 < m; i++) {
            const uint32_t ri = p.order[g0 + i];
            for (uint64_t j = i + 1; j < m; j++) rb_tsel_pair(p, ri, p.order[g0 + j], i * m + j, b, n_pairs);
        }
    }
    // big groups of this wave: all lanes on one group at a time (lane l takes the pairs whose j is l mod 64)
    unsigned long long big = __ballot(live && m > RB_TS_BIG);
    while (big) {
        const int src = __builtin_ctzll(big);
        big &= big - 1ull;
        const uint64_t bg0 = __shfl(g0, src, 64), bm = __shfl(m, src, 64);
        for (uint64_t k = (uint64_t)lane; k < bm; k += 64) p.contained[p.order[bg0 + k]] = 0;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        rb_tsel_best bb = {0, 0, 0, 0};
        uint64_t np = 0;
        for (uint64_t i = 0; i + 1 < bm; i++) {
            const uint32_t ri = p.order[bg0 + i];
            for (uint64_t j = i + 1 + (uint64_t)lane; j < bm; j += 64) rb_tsel_pair(p, ri, p.order[bg0 + j], i * bm + j, bb, np);
        }
        for (int off = 32; off > 0; off >>= 1) { // the wave's best: largest overlap, then smallest scan order
            const uint64_t oov = __shfl_xor(bb.ov, off, 64), oord = __shfl_xor(bb.ord, off, 64);
            const uint32_t ol = (uint32_t)__shfl_xor((int)bb.l, off, 64), orr = (uint32_t)__shfl_xor((int)bb.r, off, 64);
            if (oov > bb.ov || (oov == bb.ov && oov != 0 && oord < bb.ord)) bb.ov = oov, bb.ord = oord, bb.l = ol, bb.r = orr;
            np += __shfl_xor(np, off, 64);
        }
        if (lane == src) b = bb, n_pairs = np;
    }
    if (!live) return;
    p.slot[g] = b.ov ? (uint64_t)p.norm[b.l].n_ops + (uint64_t)p.norm[b.r].n_ops : 0ull;
    // has: 1 for a group with a pair, and in the high half the pairs the group leaves for a later pass (one pair per name and pass, :266-284):
    // the scan that gives the pairs their dense slots sums those as well (no atomic: 2.5e6 adds to one word were most of a pass's selection)
    // (a group's share is capped at (2^32 - 1) / n_groups so that the sum cannot leave its 32 bits: n_deferred is 0 exactly when nothing is left,
    //  and the exact count whenever no single group leaves more than that)
    const uint64_t dcap = 0xFFFFFFFFull / p.n_groups, dleft = n_pairs > 1 ? n_pairs - 1 : 0ull;
    p.has[g] = (b.ov ? 1ull : 0ull) | ((dleft < dcap ? dleft : dcap) << 32);
    p.cand[2 * g] = b.l, p.cand[2 * g + 1] = b.r;
}
// The same selection for groups of up to 16 records, a group per ROW of 16 lanes (round 6): lane j holds record j of the group -- ONE read of its
// norm row, where the thread-per-group form above walks every pair with four strided loads --, the outer index i runs row-uniform, record i's
// span reaches the lanes by ds_bpermute, lane j keeps the best pair (i, j) it has seen, and the row's best (largest overlap, then the smallest
// scan order i m + j) falls out of four rotate-and-compare steps.  Groups of more than 16 records are left to the kernel above.
__global__ __launch_bounds__(256) void rb_k_trim_select_rows(rb_tsel_params p) {
    const int lane = rb_lane();
    const uint32_t gbase = (uint32_t)lane & 48u, gl = (uint32_t)lane & 15u;
    const uint64_t g = ((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6)) * 4u + ((uint32_t)lane >> 4);
    const bool live = g < p.n_groups;
    const uint64_t g0 = live ? p.grp_off[g] : 0, m64 = live ? p.grp_off[g + 1] - g0 : 0;
    const bool mine = live && m64 <= 16u; // (row-uniform)
    const uint32_t m = mine ? (uint32_t)m64 : 0u;
    const bool have = gl < m;
    const uint32_t r = have ? p.order[g0 + gl] : 0u;
    uint64_t st = 0, en = 0;
    if (have) st = p.norm[r].q_st, en = p.norm[r].q_en;
    bool cont = false;
    rb_tsel_best b = {0, 0, 0, 0};
    uint32_t np = 0; // candidate pairs this lane has seen as their j
    uint32_t w_m = m; // (the wavefront walks as far as its largest group)
#pragma unroll
    for (int off = 16; off < 64; off <<= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)w_m, off, 64);
        w_m = w_m > o ? w_m : o;
    }
    w_m = rb_first(w_m);
    for (uint32_t i = 0; i + 1u < w_m; i++) {
        // record i of every row's group, to all lanes of the row (rows whose group is shorter see zeros and have no lane behind i)
        const uint32_t ri = rb_row_read(r, gbase, i);
        const uint64_t st1 = ((uint64_t)rb_row_read((uint32_t)(st >> 32), gbase, i) << 32) | rb_row_read((uint32_t)st, gbase, i);
        const uint64_t en1 = ((uint64_t)rb_row_read((uint32_t)(en >> 32), gbase, i) << 32) | rb_row_read((uint32_t)en, gbase, i);
        const bool pair = have && gl > i && i + 1u < m;
        const uint64_t mn = en1 < en ? en1 : en, mx = st1 > st ? st1 : st;
        const bool ovl = pair && mn > mx;                      // bed.rs:74-85
        const uint64_t ov = ovl ? mn - mx : 0;
        const bool c2 = ovl && ov == en - st;                  // paf.rs:244-249: record j is contained
        const bool c1 = ovl && !c2 && ov == en1 - st1;         // ... record i is
        cont |= c2;
        if (rb_row_ballot(c1, gbase) != 0u && gl == i) cont = true;
        if (ovl && !c2 && !c1) {
            np++;
            const uint64_t ord = (uint64_t)i * m + gl;
            if (ov > b.ov || (ov == b.ov && ord < b.ord)) {
                b.ov = ov, b.ord = ord;
                if (st1 <= st) b.l = ri, b.r = r; // the smaller q_st is "left" (:252-256)
                else b.l = r, b.r = ri;
            }
        }
    }
    // the row's best pair and its number of candidates
    uint32_t np_row = rb_row_sum(np);
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) {
        const uint64_t oov = ((uint64_t)rb_row_ror((uint32_t)(b.ov >> 32), off) << 32) | rb_row_ror((uint32_t)b.ov, off);
        const uint64_t oord = ((uint64_t)rb_row_ror((uint32_t)(b.ord >> 32), off) << 32) | rb_row_ror((uint32_t)b.ord, off);
        const uint32_t ol = rb_row_ror(b.l, off), orr = rb_row_ror(b.r, off);
        if (oov > b.ov || (oov == b.ov && oov != 0 && oord < b.ord)) b.ov = oov, b.ord = oord, b.l = ol, b.r = orr;
    }
    if (have) p.contained[r] = cont ? 1 : 0;
    if (mine && gl == 0u) {
        p.slot[g] = b.ov ? (uint64_t)p.norm[b.l].n_ops + (uint64_t)p.norm[b.r].n_ops : 0ull;
        const uint64_t dcap = 0xFFFFFFFFull / p.n_groups, dleft = np_row > 1u ? np_row - 1u : 0u; // (the cap: rb_k_trim_select)
        p.has[g] = (b.ov ? 1ull : 0ull) | ((dleft < dcap ? dleft : dcap) << 32); // (high half: pairs left for a later pass)
        p.cand[2 * g] = b.l, p.cand[2 * g + 1] = b.r;
    }
}
__global__ __launch_bounds__(256) void rb_k_trim_place(rb_tsel_params p) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= p.n_groups) return;
    const uint64_t h0 = p.has[g], h1 = p.has[g + 1]; // scanned: low half = pairs in front of the group, high half = deferred pairs in front of it
    const uint64_t k = h0 & 0xFFFFFFFFull, k1 = h1 & 0xFFFFFFFFull;
    if (g + 1 == p.n_groups) p.pass->n_pairs = k1, p.pass->n_deferred = h1 >> 32, p.pass->ops_end = p.out_base + p.slot[g + 1];
    if (k1 == k) return; // no pair in this group
    p.left[k] = p.cand[2 * g], p.right[k] = p.cand[2 * g + 1];
    p.pair_out_off[k] = p.out_base + p.slot[g];
}
// the worst status of a pass's pair rows (0 = every pair was cut), for the host's one read per pass
__global__ __launch_bounds__(256) void rb_k_trim_check(const rb_pair_row *rows, uint64_t n_pairs, rb_trim_pass *pass) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n_pairs && rows[k].status != RB_ST_OK) atomicMax(&pass->bad_status, rows[k].status);
}
extern "C" hipError_t rb_launch_trim_select(const rb_tsel_params *p, uint64_t *block_sums, hipStream_t stream) {
    hipError_t e = rb_fill_async(p->pass, 0, sizeof(rb_trim_pass), stream); // (the library's own fill kernel: capi.hip says why)
    if (e != hipSuccess) return e;
    if (p->n_groups == 0) return hipSuccess;
    const unsigned blocks = (unsigned)((p->n_groups + 255) / 256);
    hipLaunchKernelGGL(rb_k_trim_select_rows, dim3((unsigned)((p->n_groups + 15) / 16)), dim3(256), 0, stream, *p);
    hipLaunchKernelGGL(rb_k_trim_select, dim3(blocks), dim3(256), 0, stream, *p);
    e = rb_launch_exclusive_scan(p->slot, p->n_groups, block_sums, nullptr, stream);
    if (e != hipSuccess) return e;
    e = rb_launch_exclusive_scan(p->has, p->n_groups, block_sums, nullptr, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rb_k_trim_place, dim3(blocks), dim3(256), 0, stream, *p);
    return hipGetLastError();
}
extern "C" hipError_t rb_launch_trim_check(const rb_pair_row *rows, uint64_t n_pairs, rb_trim_pass *pass, hipStream_t stream) {
    if (n_pairs == 0) return hipSuccess;
    hipLaunchKernelGGL(rb_k_trim_check, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, stream, rows, n_pairs, pass);
    return hipGetLastError();
}
