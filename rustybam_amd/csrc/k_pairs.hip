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
// The same passes over the RECORDS of a batch (rb_dev_pairs_records: `rb orient [--scaffold]` and `rb filter` on a file's records) follow the row
// kernels: rb_k_pairs_rec_sum / _keys / _flag / _place.  The run-summing loop is stated once, rb_pairs_sum_runs, for both sum kernels.
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

// The run-summing loop of both sum kernels (rows here, records below), stated once.  N sums per key.  `src(k, key, s, decl)` says what item k
// (a row, a record) adds: its key -- RB_PAIRS_NOKEY: it takes no part, s is then all zero -- and its N addends; k may lie behind n.  A wavefront
// walks RB_PAIRS_ITER groups of 64 consecutive items from wave0 on; sums[i][key] takes a run's i-th sum with one atomic (none for a sum of
// 0).  Returns the OR of decl over the wavefront's items, in every lane.
template <int N, typename Src>
__device__ __forceinline__ uint32_t rb_pairs_sum_runs(const Src &src, uint64_t wave0, uint64_t n, unsigned long long *const (&sums)[N]) {
    const int lane = rb_lane();
    auto add = [&](uint64_t key, const uint64_t (&s)[N]) {
        if (key == RB_PAIRS_NOKEY) return;
#pragma unroll
        for (int i = 0; i < N; i++)
            if (s[i]) atomicAdd(&sums[i][key], (unsigned long long)s[i]); // (two's complement: orient is the i64 sum of paf.rs:124-128)
    };
    // the run that was still open at lane 63 of the last group (wave-uniform)
    uint64_t c_key = RB_PAIRS_NOKEY, c[N];
#pragma unroll
    for (int i = 0; i < N; i++) c[i] = 0;
    uint32_t decl_all = 0;
    for (int it = 0; it < RB_PAIRS_ITER; it++) {
        const uint64_t k0 = wave0 + (uint64_t)it * 64u;
        if (k0 >= n) break; // (wave-uniform)
        uint32_t decl;
        uint64_t key, s[N];
        src(k0 + lane, key, s, decl);
        decl_all |= decl;
        // runs of one key among the lanes: a lane starts one when the lane below it holds another key (an item that takes no part is a run of
        // its own with nothing to add, so a run cut by such items is two runs)
        const uint64_t below = __shfl_up(key, 1, 64);
        const bool head = lane == 0 || below != key;
        const unsigned long long heads = rb_ballot(head);
        const int start = 63 - __builtin_clzll(heads & (~0ull >> (63 - lane))); // the head of this lane's run
        // the open run goes on in lane 0, or ends here
        const uint64_t key0 = rb_readlane<uint64_t>(key, 0);
        if (key0 == c_key) {
            if (lane == 0) {
#pragma unroll
                for (int i = 0; i < N; i++) s[i] += c[i];
            }
        } else if (lane == 0) {
            add(c_key, c);
        }
        // inclusive sums inside every run
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            uint64_t u[N];
#pragma unroll
            for (int i = 0; i < N; i++) u[i] = __shfl_up(s[i], off, 64);
            if (lane - off >= start) {
#pragma unroll
                for (int i = 0; i < N; i++) s[i] += u[i];
            }
        }
        // a run's last lane holds its sums: lane 63's run stays open, the others are added now
        const bool tail = lane == 63 || ((heads >> (lane + 1)) & 1ull);
        if (tail && lane != 63) add(key, s);
        c_key = rb_readlane<uint64_t>(key, 63);
#pragma unroll
        for (int i = 0; i < N; i++) c[i] = rb_readlane<uint64_t>(s[i], 63);
    }
    if (lane == 0) add(c_key, c);
    return rb_wave_or_u32(decl_all);
}

// what a hit row adds: orient, tspan, fspan
struct rb_pairs_row_src {
    const rb_pairs_params &p;
    __device__ __forceinline__ void operator()(uint64_t k, uint64_t &key, uint64_t (&s)[3], uint32_t &decl) const {
        const rb_pairs_row w = rb_pairs_look(p, k, decl);
        key = w.key;
        s[0] = (p.mode & RB_PAIRS_ORIENT) ? (w.minus ? 0 - w.q_span : w.q_span) : 0;
        s[1] = w.t_span;
        s[2] = ((p.mode & RB_PAIRS_FILTER) && w.pass) ? w.t_span : 0;
        if (w.key == RB_PAIRS_NOKEY) s[0] = s[1] = s[2] = 0;
    }
};
__global__ __launch_bounds__(256) void rb_k_pairs_sum(rb_pairs_params p) {
    const uint64_t wave0 = ((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6)) * RB_PAIRS_WAVE_ROWS;
    unsigned long long *const sums[3] = {p.orient, p.tspan, p.fspan};
    const uint32_t decl = rb_pairs_sum_runs<3>(rb_pairs_row_src{p}, wave0, p.n_rows, sums);
    if (decl && rb_lane() == 0) atomicOr(&p.info->declined, decl);
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

// ---- the same over the RECORDS of a batch (rb_dev_pairs_records: `rb orient [--scaffold]` and `rb filter` on records) -----------------
// A lane per record, the columns read as they lie (consecutive lanes, consecutive words).  A fourth sum per key, order = sum of
// (w * (t_st + t_en)) / 2 with w = t_en - t_st, product and sum mod 2^64 (paf.rs:131-135): key_order = order / tspan is what --scaffold
// sorts by.  Orient's sums see every record that takes part, the filter's only the records that pass Q and A.
struct rb_pairs_rec {
    uint64_t key; // RB_PAIRS_NOKEY: the record takes no part
    uint64_t q_len, t_st, t_span, q_st, q_en;
    bool minus, pass;
};
__device__ __forceinline__ rb_pairs_rec rb_pairs_rec_look(const rb_pairs_rec_params &p, uint64_t r, uint32_t &decl) {
    rb_pairs_rec w;
    w.key = RB_PAIRS_NOKEY, w.q_len = 0, w.t_st = 0, w.t_span = 0, w.q_st = 0, w.q_en = 0, w.minus = false, w.pass = false;
    decl = 0;
    if (r >= p.n_rec) return w;
    w.q_st = p.q_st[r], w.q_en = p.q_en[r]; // (the placing pass copies them for a record that takes no part too)
    const uint64_t key = p.rec_key[r];
    if (key >= p.n_keys) {
        decl = RB_PAIRS_DECL_KEY;
        return w;
    }
    w.key = key;
    w.q_len = p.rec_q_len[r];
    w.minus = p.strand[r] == (uint8_t)'-';
    w.t_st = p.t_st[r];
    w.t_span = p.t_en[r] - w.t_st;
    w.pass = !(p.mode & RB_PAIRS_FILTER) || (w.q_len > p.min_query && w.t_span > p.min_aln); // main.rs:242-243, both strict
    return w;
}
// what a record adds: orient, tspan, fspan, order
struct rb_pairs_rec_src {
    const rb_pairs_rec_params &p;
    __device__ __forceinline__ void operator()(uint64_t r, uint64_t &key, uint64_t (&s)[4], uint32_t &decl) const {
        const rb_pairs_rec w = rb_pairs_rec_look(p, r, decl);
        const bool orient = (p.mode & RB_PAIRS_ORIENT) != 0;
        const uint64_t q_span = w.q_en - w.q_st;
        key = w.key;
        s[0] = orient ? (w.minus ? 0 - q_span : q_span) : 0;
        s[1] = w.t_span;
        s[2] = ((p.mode & RB_PAIRS_FILTER) && w.pass) ? w.t_span : 0;
        s[3] = orient ? (w.t_span * (w.t_st + (w.t_st + w.t_span))) >> 1 : 0; // paf.rs:133: (w * (t_st + t_en)) / 2, mod 2^64
        if (w.key == RB_PAIRS_NOKEY) s[0] = s[1] = s[2] = s[3] = 0;
    }
};
__global__ __launch_bounds__(256) void rb_k_pairs_rec_sum(rb_pairs_rec_params p) {
    const uint64_t wave0 = ((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6)) * RB_PAIRS_WAVE_ROWS;
    unsigned long long *const sums[4] = {p.orient, p.tspan, p.fspan, p.order};
    const uint32_t decl = rb_pairs_sum_runs<4>(rb_pairs_rec_src{p}, wave0, p.n_rec, sums);
    if (decl && rb_lane() == 0) atomicOr(&p.info->declined, decl);
}

__global__ __launch_bounds__(256) void rb_k_pairs_rec_keys(rb_pairs_rec_params p) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= p.n_keys) return;
    p.key_flip[i] = (long long)p.orient[i] < 0 ? 1 : 0; // paf.rs:146: a sum of exactly 0 stays as it is
    // paf.rs:143.  (a key without records has tspan 0 as well: whether a span of 0 is the reference's panic is the flag pass's to say)
    if (p.key_order) p.key_order[i] = ((p.mode & RB_PAIRS_ORIENT) && p.tspan[i] != 0) ? p.order[i] / p.tspan[i] : 0;
}

// One lane per record: cnt[] as in rb_k_pairs_flag -- 1 for a record that stays, 1 << 32 more if its key is flipped --, and the two reasons to
// decline that only the finished sums show
__global__ __launch_bounds__(256) void rb_k_pairs_rec_flag(rb_pairs_rec_params p) {
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const int lane = rb_lane();
    uint32_t decl;
    const rb_pairs_rec w = rb_pairs_rec_look(p, r, decl); // (what the sum pass declined for is already in info)
    decl = 0;
    bool keep = false, flip = false;
    if (w.key != RB_PAIRS_NOKEY) {
        flip = p.key_flip[w.key] != 0;
        if ((p.mode & RB_PAIRS_ORIENT) && p.tspan[w.key] == 0) decl |= RB_PAIRS_DECL_ZERO_SPAN; // paf.rs:143 divides by it
        if (flip && w.q_len < w.q_en) decl |= RB_PAIRS_DECL_WRAP;                               // paf.rs:148 wraps (or panics, by the build)
        keep = w.pass && (!(p.mode & RB_PAIRS_FILTER) || p.paired_len < p.fspan[w.key]);        // paf.rs:100, strict
    }
    if (r < p.n_rec) p.cnt[r] = keep ? (1ull | ((uint64_t)(flip ? 1 : 0) << 32)) : 0ull;
    decl = rb_wave_or_u32(decl);
    if (decl && lane == 0) atomicOr(&p.info->declined, decl);
}

// One lane per record: its index goes to its place among the kept ones, its query coordinates -- flipped where its key is (paf.rs:148-151) --
// to the two columns
__global__ __launch_bounds__(256) void rb_k_pairs_rec_place(rb_pairs_rec_params p) {
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (r == 0) { // the totals, exact whatever kept_cap
        const uint64_t total = p.cnt[p.n_rec];
        p.info->n_kept = (uint32_t)total, p.info->n_flipped_rows = total >> 32;
    }
    if (r >= p.n_rec) return;
    const uint32_t dst = (uint32_t)p.cnt[r]; // (the low half: kept records in front of this one; cnt[n_rec] is the total)
    if ((uint32_t)p.cnt[r + 1] != dst) {
        if (dst < p.kept_cap) p.kept[dst] = (uint32_t)r;
        else atomicOr(&p.info->overflow, 1u); // (n_kept stays exact: it is the scan's total)
    }
    if (!p.q_st_out) return;
    uint64_t q_st = p.q_st[r], q_en = p.q_en[r];
    const uint64_t key = p.rec_key[r];
    if (key < p.n_keys && p.key_flip[key]) {
        const uint64_t q_len = p.rec_q_len[r];
        const uint64_t n_st = q_len - q_en, n_en = q_len - q_st;
        q_st = n_st, q_en = n_en;
    }
    p.q_st_out[r] = q_st, p.q_en_out[r] = q_en;
}

// the sums and info are zeroed by the caller on the same stream
extern "C" hipError_t rb_launch_pairs_records(const rb_pairs_rec_params *p, uint64_t *block_sums, hipStream_t stream) {
    if (p->n_rec) hipLaunchKernelGGL(rb_k_pairs_rec_sum, dim3((unsigned)((p->n_rec + RB_PAIRS_BLOCK_ROWS - 1) / RB_PAIRS_BLOCK_ROWS)), dim3(256), 0, stream, *p);
    if (p->n_keys) hipLaunchKernelGGL(rb_k_pairs_rec_keys, dim3((unsigned)((p->n_keys + 255) / 256)), dim3(256), 0, stream, *p); // (no records: nothing flips)
    if (p->n_rec == 0) return hipGetLastError();
    hipLaunchKernelGGL(rb_k_pairs_rec_flag, dim3((unsigned)((p->n_rec + 255) / 256)), dim3(256), 0, stream, *p);
    const hipError_t e = rb_launch_exclusive_scan(p->cnt, p->n_rec, block_sums, nullptr, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rb_k_pairs_rec_place, dim3((unsigned)((p->n_rec + 255) / 256)), dim3(256), 0, stream, *p);
    return hipGetLastError();
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
