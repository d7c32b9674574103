// k_rows_batch.hip -- the hit rows of a clip call as a dense batch of records (gfx950, wave64): rb_dev_rows_to_batch.
//
// The link between two clip calls: `rb break-paf .. | rb liftover ..` without the text in between.  What the first call leaves is hit
// rows whose clips lie scattered in out_ops or are 4-word descriptors into the batch (RB_LIFT_DESCRIPTORS); what the second call takes is
// a batch view.  Every row with status RB_ST_OK becomes one record ("piece") of the new batch, in row order; its ops are the clip's ops
// under the rules of rb_hs_locate (k_hitstats.hip), its coordinates the row's, its strand and contig the parent record's.
//
// Shape.  Three steps on the stream, no global atomic decides a place, so two calls write the same bytes:
//   rb_k_rtb_count  a thread per row: the clip's op count and a 1 per OK row into two u64 arrays; a panic status or a replaced length that
//                   no longer fits 28 bits sets info->declined (an OR: it places nothing).
//   the device-wide exclusive scan of both arrays (the three small launches every scan of this library takes): where a piece's ops and
//                   its header go, and the exact totals, capacities or not.
//   rb_k_rtb_fill   the copy, shaped as rb_k_hitstats: a clip is a ROW of 16 lanes, four clips to a wavefront, a row's step RB_RTB_ROW_STEP
//                   = 64 ops, RB_RTB_BATCH steps in flight together; a clip of more than RB_RTB_ROW_MAX ops is left out by the row form and
//                   walked afterwards by the SAME wavefront with all 64 lanes (RB_RTB_WAVE_STEP = 256 ops, 1 KiB per instruction).
//
// Which side is aligned: BOTH.  A piece's destination new_ops + new_op_off[p] is rarely 16-byte aligned with its source, but the source
// must be read in whole aligned 16-byte groups (the memory contract: nothing but groups that hold a word of the clip is touched, and the
// record's neighbours in a slot are somebody else's), and the destination is where width pays most: a store is issued per instruction, a
// dword store moves a quarter of the bytes of a dwordx4 for the same issue slot, and a 16-byte store that straddles two 16-byte groups is
// split on its way.  So a lane that holds source group G builds DESTINATION group G from its own words and the last three words of the
// lane in front of it (one DPP move each; across steps the row's / wavefront's last lane carries them): with sh = (destination - source)
// mod 4 words, destination group G is source words 4G - sh .. 4G + 3 - sh.  Interior groups are stored with one aligned dwordx4; only a
// clip's first and last group (shared with the neighbouring pieces, which other lanes write) are stored word by word.
//
// Lengths of 2^28 and more.  A clip's words are copied as WORDS: an op and the RB_OP_CONT word behind it arrive together, so clips that
// hold continuation words (plain ops of the generic kernel; no clip kernel writes a descriptor over a record that has one) are handled.
// A descriptor's replaced first / last length is one word's worth: if it is 2^28 or more the piece would need a word it has no place
// for, and the call DECLINES (info->declined; the word then holds the low 28 bits).
//
// Memory.  Reads: the rows, aligned 16-byte groups that hold a word of a clip or of a descriptor, op_off / strand / contig of the rows'
// records.  Writes: new_ops[0 .. n_ops), the per-piece arrays [0 .. n_pieces), new_op_off[0 .. n_pieces], info -- each only below its
// capacity.  Roofline: 64 B per row, 8 B per op (4 read, 4 written), 54 B of header per piece (49 written, the parent's strand and
// contig read; + 16 B per descriptor).
#include "rb_device.h"
#include "rb_launch.h"

#define RB_RTB_ROW_STEP 64u   // ops per step of a row of 16 lanes (one 16-byte group per lane)
#define RB_RTB_WAVE_STEP 256u // ops per step of the whole wavefront (long clips)
#ifndef RB_RTB_ROW_MAX
#define RB_RTB_ROW_MAX 4096u  // clips of more ops than this take the wavefront form (rb_k_hitstats' line: same clips, same spread)
#endif
#ifndef RB_RTB_BATCH
#define RB_RTB_BATCH 4        // steps whose loads are in flight together
#endif

extern "C" uint32_t rb_rtb_row_step(void) { return RB_RTB_ROW_STEP; }
extern "C" uint32_t rb_rtb_wave_step(void) { return RB_RTB_WAVE_STEP; }
extern "C" uint32_t rb_rtb_row_max(void) { return RB_RTB_ROW_MAX; }

struct rb_rtb_clip {
    const uint32_t *gsrc; // the aligned group that holds the clip's first word
    uint32_t head;        // words of that group in front of the clip (0 .. 3)
    uint32_t n;           // words of the clip
    uint32_t fl, ll;      // descriptor rows: != 0 replaces the length of the first / last op
};

// where the clip of an RB_ST_OK row lies: rb_hs_locate's rules (k_hitstats.hip)
__device__ __forceinline__ rb_rtb_clip rb_rtb_locate(const rb_rows_batch_params &p, const rb_hit_row &h) {
    rb_rtb_clip c;
    const uint32_t *src = p.out_ops + h.out_off;
    c.n = h.out_n;
    c.fl = c.ll = 0u;
    if (h.flags & RB_HIT_DESCRIPTOR) {
        const uint4 d = rb_load4_unaligned(src); // (the descriptor's own 16 bytes, wherever out_off puts them; the clip kernels: 4 * row)
        c.n = d.y;
        if (!(h.flags & RB_HIT_INSIDE)) c.fl = d.z, c.ll = d.w;
        src = p.ops + p.op_off[h.rec] + d.x; // (op_off as a table of starts)
    }
    c.head = (uint32_t)(((uintptr_t)src >> 2) & 3u);
    c.gsrc = src - c.head;
    return c;
}

// ---- step 1: the counts the scans turn into places -------------------------------------------------
__global__ __launch_bounds__(256) void rb_k_rtb_count(rb_rows_batch_params p) {
    const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (k >= p.n_rows) return;
    const rb_hit_row *row = p.rows + k;
    const uint4 hd = *reinterpret_cast<const uint4 *>(row); // rec, win, status | flags << 16, out_n
    const uint32_t status = hd.z & 0xFFFFu, flags = hd.z >> 16;
    uint64_t n = 0;
    bool bad = status >= (uint32_t)RB_ST_PANIC_NOTFOUND;
    if (status == RB_ST_OK) {
        n = hd.w;
        if (flags & RB_HIT_DESCRIPTOR) {
            const uint32_t *dsc = p.out_ops + row->out_off;
            const uint4 d = rb_load4_unaligned(dsc);
            n = d.y;
            if (!(flags & RB_HIT_INSIDE)) {
                if (d.y == 1u && d.z && d.w) {
                    const uint32_t len = p.ops[p.op_off[hd.x] + d.x] >> 4;
                    bad |= (uint32_t)(d.z + d.w - len) > RB_LEN_MASK_WORD;
                } else
                    bad |= d.z > RB_LEN_MASK_WORD || d.w > RB_LEN_MASK_WORD;
            }
        }
    }
    p.cnt_ops[k] = n;
    p.cnt_pieces[k] = status == RB_ST_OK ? 1ull : 0ull;
    if (bad) atomicOr(&p.info->declined, 1u);
}

// ---- step 3: the copy ---------------------------------------------------------------------------------
// One clip by W lanes (16: a row, every row of the wavefront its own clip; 64: the wavefront).  d0 = index in new_ops of the clip's first
// word.  Coordinates: e = source coordinate (counted from gsrc) + sh, so that e and the destination index agree mod 4; the clip is
// e in [e0, e1), destination group G = e in [4G, 4G + 4) lies at new_ops + dbase + 4G.
template <int W>
__device__ __forceinline__ void rb_rtb_walk(const rb_rtb_clip &c, const bool take, const uint64_t d0, uint32_t *new_ops, const uint64_t ops_cap,
                                            const int lane) {
    static_assert((W == 16 && 4 * W == RB_RTB_ROW_STEP) || (W == 64 && 4 * W == RB_RTB_WAVE_STEP), "a step is one 16-byte group per lane");
    const uint32_t gl = (uint32_t)lane & (uint32_t)(W - 1);
    const uint32_t n = c.n;
    const uint32_t sh = ((uint32_t)d0 - c.head) & 3u;
    const uint64_t e0 = (uint64_t)c.head + sh, e1 = e0 + n;
    const int64_t dbase = (int64_t)d0 - (int64_t)e0; // a multiple of 4 (-4 at the least)
    const bool one_both = n == 1u && c.fl && c.ll;
    const bool live = take && n != 0u;
    const uint32_t n_steps = live ? (uint32_t)((e1 + (4u * W - 1u)) / (4u * W)) : 0u;
    const uint64_t last_off = live ? (((uint64_t)c.head + n - 1u) & ~3ull) : 0ull;
    uint32_t w_steps = n_steps; // the wavefront's steps: the longest of its clips
    if (W == 16) {
#pragma unroll
        for (int off = 16; off < 64; off <<= 1) {
            const uint32_t o = (uint32_t)__shfl_xor((int)w_steps, off, 64);
            w_steps = w_steps > o ? w_steps : o;
        }
    }
    w_steps = rb_first(w_steps);
    uint32_t cy = 0u, cz = 0u, cw = 0u; // the last three words of the group in front of this step's first one
    for (uint32_t b0 = 0; b0 < w_steps; b0 += RB_RTB_BATCH) {
        uint4 pf[RB_RTB_BATCH];
#pragma unroll
        for (int s = 0; s < RB_RTB_BATCH; s++) {
            uint64_t off = (uint64_t)(b0 + (uint32_t)s) * (4u * W) + gl * 4u;
            off = off < last_off ? off : last_off; // (past the clip's last group: that group again; its words are masked below)
            pf[s] = live ? *reinterpret_cast<const uint4 *>(c.gsrc + off) : make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (int s = 0; s < RB_RTB_BATCH; s++) {
            const uint32_t st = b0 + (uint32_t)s;
            if (st >= w_steps) break; // (uniform)
            const uint4 v = pf[s];
            uint32_t py, pz, pw; // words 1 .. 3 of the source group in front of mine
            if (W == 16) {
                py = (uint32_t)__builtin_amdgcn_update_dpp((int)cy, (int)v.y, RB_DPP_ROW_SHR(1), 0xf, 0xf, false);
                pz = (uint32_t)__builtin_amdgcn_update_dpp((int)cz, (int)v.z, RB_DPP_ROW_SHR(1), 0xf, 0xf, false);
                pw = (uint32_t)__builtin_amdgcn_update_dpp((int)cw, (int)v.w, RB_DPP_ROW_SHR(1), 0xf, 0xf, false);
                cy = rb_row_last(v.y), cz = rb_row_last(v.z), cw = rb_row_last(v.w);
            } else {
                py = rb_prev_lane(v.y, cy), pz = rb_prev_lane(v.z, cz), pw = rb_prev_lane(v.w, cw);
                cy = rb_readlane<uint32_t>(v.y, 63), cz = rb_readlane<uint32_t>(v.z, 63), cw = rb_readlane<uint32_t>(v.w, 63);
            }
            if (st < n_steps) { // (uniform over the W lanes: a row whose clip has ended sits the step out)
                uint32_t o[4]; // destination group G = source words 4G - sh .. 4G + 3 - sh
                o[0] = sh == 0u ? v.x : sh == 1u ? pw : sh == 2u ? pz : py;
                o[1] = sh == 0u ? v.y : sh == 1u ? v.x : sh == 2u ? pw : pz;
                o[2] = sh == 0u ? v.z : sh == 1u ? v.y : sh == 2u ? v.x : pw;
                o[3] = sh == 0u ? v.w : sh == 1u ? v.z : sh == 2u ? v.y : v.x;
                const uint64_t eg = (uint64_t)st * (4u * W) + gl * 4u; // e of o[0]
                const int64_t dg = dbase + (int64_t)eg;                // index of o[0] in new_ops
                if (eg > e0 && eg + 4u < e1 && (uint64_t)dg + 4u <= ops_cap) { // an interior group: neither the first nor the last word is in it
                    *reinterpret_cast<uint4 *>(new_ops + dg) = make_uint4(o[0], o[1], o[2], o[3]);
                } else {
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const uint64_t e = eg + (uint32_t)q;
                        if (e < e0 || e >= e1) continue;
                        const uint32_t idx = (uint32_t)(e - e0);
                        uint32_t w = o[q], len = w >> 4;
                        if (one_both) len = c.fl + c.ll - len; // (idx == 0 is the only word there is)
                        else {
                            if (idx == 0u && c.fl) len = c.fl;
                            if (idx == n - 1u && c.ll) len = c.ll;
                        }
                        w = ((len & RB_LEN_MASK_WORD) << 4) | (w & 15u);
                        if ((uint64_t)(dg + q) < ops_cap) new_ops[dg + q] = w;
                    }
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void rb_k_rtb_fill(rb_rows_batch_params p) {
    const int lane = rb_lane();
    const uint32_t gl = (uint32_t)lane & 15u;
    const uint64_t k0 = ((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6)) * 4u; // the wavefront's first row
    const uint64_t k = k0 + ((uint32_t)lane >> 4);
    const bool in = k < p.n_rows;
    rb_hit_row h;
    h.status = 0xFFFFu, h.flags = 0, h.out_n = 0, h.out_off = 0, h.rec = 0;
    h.t_st = h.t_en = h.q_st = h.q_en = 0;
    if (in) h = p.rows[k];
    const bool ok = in && h.status == RB_ST_OK;
    rb_rtb_clip c;
    c.gsrc = p.out_ops, c.head = 0u, c.n = 0u, c.fl = c.ll = 0u;
    uint64_t d0 = 0;
    if (ok) {
        c = rb_rtb_locate(p, h);
        d0 = p.cnt_ops[k]; // (scanned: where the piece's ops go)
        const uint64_t pc = p.cnt_pieces[k];
        if (gl == 0u && pc < p.pieces_cap) { // the piece's header
            p.new_op_off[pc] = d0;
            p.t_st[pc] = h.t_st, p.t_en[pc] = h.t_en, p.q_st[pc] = h.q_st, p.q_en[pc] = h.q_en;
            p.strand[pc] = p.src_strand[h.rec];
            p.contig[pc] = p.src_contig[h.rec];
            p.parent[pc] = h.rec;
        }
    }
    if (k == 0 && gl == 0u) { // the totals (the scans left them behind the counts), once
        const uint64_t n_pieces = p.cnt_pieces[p.n_rows], n_ops = p.cnt_ops[p.n_rows];
        if (n_pieces <= p.pieces_cap) p.new_op_off[n_pieces] = n_ops;
        if (n_pieces > p.pieces_cap || n_ops > p.ops_cap) p.info->overflow = 1u;
    }
    const bool is_long = ok && c.n > RB_RTB_ROW_MAX;
    rb_rtb_walk<16>(c, ok && !is_long, d0, p.new_ops, p.ops_cap, lane);
    // ---- the long clips of these four rows, one after the other, by the whole wavefront ----
    unsigned long long todo = rb_ballot(is_long && gl == 0u);
    while (todo) {
        const uint32_t b = (uint32_t)__builtin_ctzll(todo);
        todo &= todo - 1ull;
        const uint64_t kk = k0 + (b >> 4);
        const rb_hit_row hl = p.rows[kk];
        const rb_rtb_clip cl = rb_rtb_locate(p, hl);
        rb_rtb_walk<64>(cl, true, p.cnt_ops[kk], p.new_ops, p.ops_cap, lane);
    }
}

extern "C" hipError_t rb_launch_rows_batch_count(const rb_rows_batch_params *p, hipStream_t stream) {
    if (p->n_rows == 0) return hipSuccess;
    hipLaunchKernelGGL(rb_k_rtb_count, dim3((unsigned)((p->n_rows + 255) / 256)), dim3(256), 0, stream, *p);
    return hipGetLastError();
}
extern "C" hipError_t rb_launch_rows_batch_fill(const rb_rows_batch_params *p, hipStream_t stream) {
    if (p->n_rows == 0) return hipSuccess;
    hipLaunchKernelGGL(rb_k_rtb_fill, dim3((unsigned)((p->n_rows + 15) / 16)), dim3(256), 0, stream, *p);
    return hipGetLastError();
}
