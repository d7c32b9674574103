// k_pairs.hip -- `rb orient` and `rb filter` (paf.rs:91-157, main.rs:234-267) over hit rows where a clip call left them, for gfx950.  Neither
// command touches a CIGAR: both are sums over the records' headers keyed by the (target name, query name) pair.  The host interns the pairs
// into dense keys per RECORD; a row's key is its record's, the device never sees a string.
//   rb_k_pairs_sum    one read of the rows feeds three integer sums per key:  orient = sum of +-(q_en - q_st) by strand and tspan = sum of
//                     (t_en - t_st), both over every row that takes part (paf.rs:119-135), and fspan = the same span over the rows that pass
//                     filter_query_len and filter_aln_len (main.rs:242-243 run in front of filter_aln_pairs, paf.rs:91-98).  None of the
//                     three depends on another: orient changes query coordinates and the strand only, the filter looks at neither.
//   rb_k_pairs_keys   key_flip[key] = orient < 0 (paf.rs:146, strict)
//   rb_k_pairs_flag   1 per kept row (and 1 << 32 per flipped one), the library's exclusive scan over those (block sums, no atomics), then
//   rb_k_pairs_place  the kept rows, dense, in row order, a flipped key's rows with q_st / q_en rewritten (paf.rs:148-151)
// Rows arrive in record order, so equal keys come in runs and a file of a few contig pairs has every row of a wavefront on one key (9 keys
// for 2447 pieces in tests/golden/asm_small.paf): a wavefront sums each run among its lanes and carries the run that is still open from one
// group of 64 rows to the next, so a run costs one 64-bit atomic per sum and wavefront -- at least RB_PAIRS_WAVE_ROWS rows apart -- not
// one per row.  The sums are integers: the result is the same in whatever order the atomics arrive, and nothing is PLACED by an atomic, so
// two calls on the same input write the same bytes.
#include "rb_device.h"
#include "rb_launch.h"

#define RB_PAIRS_ITER 8                          // groups of 64 rows a wavefront walks, one behind the other
#define RB_PAIRS_WAVE_ROWS (64 * RB_PAIRS_ITER)  // consecutive rows of one wavefront
#define RB_PAIRS_BLOCK_ROWS (4 * RB_PAIRS_WAVE_ROWS)
#define RB_PAIRS_NOKEY 0xFFFFFFFFFFFFFFFFull     // (a u64: no u32 key looks like it)

// what a row has to say: from its first three 16-byte pieces {rec, win, status | flags << 16, out_n}, {t_st, t_en}, {q_st, q_en}
struct rb_pairs_row {
    uint64_t key;   // RB_PAIRS_NOKEY: the row takes no part
    uint64_t q_len; // of its record
    uint64_t t_span, q_span;
    uint64_t q_st, q_en;
    bool minus;     // the record's strand is '-'
    bool pass;      // filter_query_len and filter_aln_len keep it (true without RB_PAIRS_FILTER)
};
// decl: the reasons this row declines the call for (RB_PAIRS_DECL_PANIC, RB_PAIRS_DECL_KEY)
__device__ __forceinline__ rb_pairs_row rb_pairs_look(const rb_pairs_params &p, uint64_t k, uint32_t &decl) {
    rb_pairs_row w;
    w.key = RB_PAIRS_NOKEY, w.q_len = 0, w.t_span = 0, w.q_span = 0, w.q_st = 0, w.q_en = 0, w.minus = false, w.pass = false;
    decl = 0;
    if (k >= p.n_rows) return w;
    const uint4 *r = reinterpret_cast<const uint4 *>(p.rows + k);
    const uint4 a = r[0], b = r[1], c = r[2];
    const uint32_t status = a.z & 0xFFFFu;
    if (status >= RB_ST_PANIC_NOTFOUND) decl = RB_PAIRS_DECL_PANIC;
    if (status != RB_ST_OK) return w; // (the reference's None: no record, it counts nowhere)
    uint64_t key = RB_PAIRS_NOKEY;
    if ((uint64_t)a.x < p.n_rec) key = p.rec_key[a.x];
    if (key >= p.n_keys) {
        decl = RB_PAIRS_DECL_KEY;
        return w;
    }
    w.key = key;
    w.q_len = p.rec_q_len[a.x];
    w.minus = p.strand[a.x] == (uint8_t)'-';
    w.t_span = (((uint64_t)b.w << 32) | b.z) - (((uint64_t)b.y << 32) | b.x);
    w.q_st = ((uint64_t)c.y << 32) | c.x, w.q_en = ((uint64_t)c.w << 32) | c.z;
    w.q_span = w.q_en - w.q_st;
    w.pass = !(p.mode & RB_PAIRS_FILTER) || (w.q_len > p.min_query && w.t_span > p.min_aln); // main.rs:242-243, both strict
    return w;
}

__device__ __forceinline__ void rb_pairs_add(const rb_pairs_params &p, uint64_t key, uint64_t o, uint64_t t, uint64_t f) {
    if (key == RB_PAIRS_NOKEY) return;
    if (o) atomicAdd(&p.orient[key], (unsigned long long)o); // (two's complement: the i64 sum of paf.rs:124-128)
    if (t) atomicAdd(&p.tspan[key], (unsigned long long)t);
    if (f) atomicAdd(&p.fspan[key], (unsigned long long)f);
}

__global__ __launch_bounds__(256) void rb_k_pairs_sum(rb_pairs_params p) {
    const int lane = rb_lane();
    const uint64_t wave0 = ((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6)) * RB_PAIRS_WAVE_ROWS;
    // the run that was still open at lane 63 of the last group (wave-uniform)
    uint64_t c_key = RB_PAIRS_NOKEY, c_o = 0, c_t = 0, c_f = 0;
    uint32_t decl_all = 0;
    for (int it = 0; it < RB_PAIRS_ITER; it++) {
        const uint64_t k0 = wave0 + (uint64_t)it * 64u;
        if (k0 >= p.n_rows) break; // (wave-uniform)
        uint32_t decl;
        const rb_pairs_row w = rb_pairs_look(p, k0 + lane, decl);
        decl_all |= decl;
        uint64_t o = (p.mode & RB_PAIRS_ORIENT) ? (w.minus ? 0 - w.q_span : w.q_span) : 0;
        uint64_t t = w.t_span;
        uint64_t f = ((p.mode & RB_PAIRS_FILTER) && w.pass) ? w.t_span : 0;
        if (w.key == RB_PAIRS_NOKEY) o = t = f = 0;
        // runs of one key among the lanes: a lane starts one when the lane below it holds another key (a row that takes no part is a run of
        // its own with nothing to add, so a run cut by such rows is two runs)
        const uint64_t below = __shfl_up(w.key, 1, 64);
        const bool head = lane == 0 || below != w.key;
        const unsigned long long heads = rb_ballot(head);
        const int start = 63 - __builtin_clzll(heads & (~0ull >> (63 - lane))); // the head of this lane's run
        // the open run goes on in lane 0, or ends here
        const uint64_t key0 = rb_readlane<uint64_t>(w.key, 0);
        if (key0 == c_key) {
            if (lane == 0) o += c_o, t += c_t, f += c_f;
        } else if (lane == 0) {
            rb_pairs_add(p, c_key, c_o, c_t, c_f);
        }
        // inclusive sums inside every run
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint64_t uo = __shfl_up(o, off, 64), ut = __shfl_up(t, off, 64), uf = __shfl_up(f, off, 64);
            if (lane - off >= start) o += uo, t += ut, f += uf;
        }
        // a run's last lane holds its sums: lane 63's run stays open, the others are added now
        const bool tail = lane == 63 || ((heads >> (lane + 1)) & 1ull);
        if (tail && lane != 63) rb_pairs_add(p, w.key, o, t, f);
        c_key = rb_readlane<uint64_t>(w.key, 63);
        c_o = rb_readlane<uint64_t>(o, 63), c_t = rb_readlane<uint64_t>(t, 63), c_f = rb_readlane<uint64_t>(f, 63);
    }
    if (lane == 0) rb_pairs_add(p, c_key, c_o, c_t, c_f);
    decl_all = rb_wave_or_u32(decl_all);
    if (decl_all && lane == 0) atomicOr(&p.info->declined, decl_all);
}

__global__ __launch_bounds__(256) void rb_k_pairs_keys(rb_pairs_params p) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < p.n_keys) p.key_flip[i] = (long long)p.orient[i] < 0 ? 1 : 0; // paf.rs:146: a sum of exactly 0 stays as it is
}

// One lane per row: cnt[] (the scan's input) = 1 for a row that stays, and 1 << 32 more if its key is flipped -- one scan then counts both, the
// kept rows in the low half and the flipped ones among them in the high half (n_rows < 2^32: no carry between the halves), where one atomic
// per wavefront on the one address in info would queue n_rows / 64 adders (measured: 1.0 of 1.9 ms on 8e6 rows) --, and the two reasons to
// decline that only the finished sums show.
__global__ __launch_bounds__(256) void rb_k_pairs_flag(rb_pairs_params p) {
    const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const int lane = rb_lane();
    uint32_t decl;
    const rb_pairs_row w = rb_pairs_look(p, k, decl); // (what the sum pass declined for is already in info)
    decl = 0;
    bool keep = false, flip = false;
    if (w.key != RB_PAIRS_NOKEY) {
        flip = p.key_flip[w.key] != 0;
        // orient() divides by the pair's target bases (paf.rs:143): a pair that has rows and no base is its panic
        if ((p.mode & RB_PAIRS_ORIENT) && p.tspan[w.key] == 0) decl |= RB_PAIRS_DECL_ZERO_SPAN;
        // paf.rs:148: q_len - q_en of a record that ends behind its query's length wraps (or panics, by the build)
        if (flip && w.q_len < w.q_en) decl |= RB_PAIRS_DECL_WRAP;
        keep = w.pass && (!(p.mode & RB_PAIRS_FILTER) || p.paired_len < p.fspan[w.key]); // paf.rs:100, strict
    }
    if (k < p.n_rows) p.cnt[k] = keep ? (1ull | ((uint64_t)(flip ? 1 : 0) << 32)) : 0ull;
    decl = rb_wave_or_u32(decl);
    if (decl && lane == 0) atomicOr(&p.info->declined, decl);
}

// Four lanes per row, one 16-byte piece each: a wavefront loads and stores 1 KiB of whole rows per instruction.  The row's first piece
// (lane 0 of the four) says which record it belongs to; the third piece holds q_st / q_en.
__global__ __launch_bounds__(256) void rb_k_pairs_place(rb_pairs_params p) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint64_t k = t >> 2;
    const int piece = (int)(t & 3u), lane = rb_lane();
    uint4 v = make_uint4(0, 0, 0, 0);
    uint64_t dst = 0;
    bool keep = false;
    if (k < p.n_rows) {
        v = reinterpret_cast<const uint4 *>(p.rows + k)[piece];
        dst = (uint32_t)p.cnt[k]; // (the low half: kept rows in front of this one)
        keep = (uint32_t)p.cnt[k + 1] != (uint32_t)dst; // (cnt is the exclusive prefix of the flags: cnt[n_rows] is the total)
    }
    if (t == 0) { // the totals, exact whatever rows_cap
        const uint64_t total = p.cnt[p.n_rows];
        p.info->n_kept = (uint32_t)total, p.info->n_flipped_rows = total >> 32;
    }
    const uint32_t rec = (uint32_t)__shfl((int)v.x, lane & ~3, 64);
    if (!keep) return;
    if (dst >= p.rows_cap) {
        if (piece == 0) atomicOr(&p.info->overflow, 1u); // (n_kept stays exact: it is the scan's total)
        return;
    }
    if (piece == 2 && p.key_flip[p.rec_key[rec]]) { // (a kept row: rec < n_rec and its key < n_keys were checked by the passes in front)
        const uint64_t q_len = p.rec_q_len[rec];
        const uint64_t q_st = ((uint64_t)v.y << 32) | v.x, q_en = ((uint64_t)v.w << 32) | v.z;
        const uint64_t n_st = q_len - q_en, n_en = q_len - q_st; // paf.rs:148-151
        v = make_uint4((uint32_t)n_st, (uint32_t)(n_st >> 32), (uint32_t)n_en, (uint32_t)(n_en >> 32));
    }
    reinterpret_cast<uint4 *>(p.rows_out + dst)[piece] = v;
}

// the descriptors of the kept rows, dense (rb_host_break_pairs_text: the text tail wants row k's at desc[4k]); zeros for a row of plain ops
__global__ __launch_bounds__(256) void rb_k_pairs_desc(const rb_hit_row *rows, uint64_t n_rows, const uint32_t *out_ops, uint4 *desc) {
    const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (k >= n_rows) return;
    const uint4 a = reinterpret_cast<const uint4 *>(rows + k)[0];
    const uint64_t out_off = rows[k].out_off;
    const bool d = (a.z & 0xFFFFu) == RB_ST_OK && ((a.z >> 16) & RB_HIT_DESCRIPTOR);
    desc[k] = d ? make_uint4(out_ops[out_off], out_ops[out_off + 1], out_ops[out_off + 2], out_ops[out_off + 3]) : make_uint4(0, 0, 0, 0);
}

extern "C" uint32_t rb_pairs_wave_rows(void) { return RB_PAIRS_WAVE_ROWS; }
extern "C" uint32_t rb_pairs_block_rows(void) { return RB_PAIRS_BLOCK_ROWS; }

// the sums and info are zeroed by the caller on the same stream
extern "C" hipError_t rb_launch_pairs(const rb_pairs_params *p, uint64_t *block_sums, hipStream_t stream) {
    if (p->n_rows) hipLaunchKernelGGL(rb_k_pairs_sum, dim3((unsigned)((p->n_rows + RB_PAIRS_BLOCK_ROWS - 1) / RB_PAIRS_BLOCK_ROWS)), dim3(256), 0, stream, *p);
    if (p->n_keys) hipLaunchKernelGGL(rb_k_pairs_keys, dim3((unsigned)((p->n_keys + 255) / 256)), dim3(256), 0, stream, *p); // (no rows: nothing flips)
    if (p->n_rows == 0) return hipGetLastError();
    hipLaunchKernelGGL(rb_k_pairs_flag, dim3((unsigned)((p->n_rows + 255) / 256)), dim3(256), 0, stream, *p);
    const hipError_t e = rb_launch_exclusive_scan(p->cnt, p->n_rows, block_sums, nullptr, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rb_k_pairs_place, dim3((unsigned)((p->n_rows * 4 + 255) / 256)), dim3(256), 0, stream, *p);
    return hipGetLastError();
}
extern "C" hipError_t rb_launch_pairs_desc(const rb_hit_row *rows, uint64_t n_rows, const uint32_t *out_ops, uint32_t *desc, hipStream_t stream) {
    if (n_rows == 0) return hipSuccess;
    hipLaunchKernelGGL(rb_k_pairs_desc, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, stream, rows, n_rows, out_ops, reinterpret_cast<uint4 *>(desc));
    return hipGetLastError();
}
