// k_liftover.hip -- liftover / break-paf clip kernels for gfx950 (wave64, CDNA4).
//
// Replaces liftover::trim_helper + trim_paf_rec_to_rgn (liftover.rs:17-132) and everything they
// call (aligned_pairs paf.rs:501-538, tpos_to_idx_match :541-561, subset_cigar /
// collapse_long_cigar :593-620).  The reference expands every CIGAR to per-base arrays (24 B per
// aligned base) and binary-searches them; here the walk stays in op space:
//
//   rb_k_count_hits     one thread per record: number of overlapping windows (paf.rs:622-627)
//   rb_k_scan_*         exclusive scan of the counts -> first row of every record (canonical order)
//   rb_k_make_jobs      one thread per schedule slot: a 64-byte job descriptor, so that a wave starts on its record
//                       after ONE load instead of a chain of dependent ones
//   rb_k_liftover_stream  ONE WAVEFRONT PER RECORD (its body: rb_stream.h).  The record's packed ops stream from HBM once (2 KiB per
//                       step, lane l the 16-byte groups l and l + 64 of it, two steps in flight in a register ring the compiler
//                       cannot see); per lane the reference / query / unit lengths of each group's 4 ops are summed (op class ->
//                       mask with one v_bfe_i32), 6-step DPP prefix scans give the running offsets, every second or
//                       fourth lane leaves a checkpoint for each half of the step in LDS; window boundaries are resolved lane-parallel against
//                       the checkpoints (lane j: start of window j, lane j + 32: its end).  Clips are emitted FROM
//                       THE LOAD RING while the record streams: output slot k mirrors the input's op positions
//                       (out_ops[k * slot_stride + 32 r + position]), clip j of a record goes to slot j mod n_slots,
//                       and a lane stores the 8 ops it has just loaded into every slot whose current clip its
//                       reference span touches -- no size is needed to place a clip, so there is no reservation,
//                       no atomic and no second read.  After the segment's resolution only the two end ops of a
//                       clip are patched (clipped first / last length).  Clips that would land within four lines of
//                       the previous clip of their slot, and clips of windows that are not sorted, are listed and
//                       copied by rb_k_copy_clips into the arenas behind the slots.
//   rb_k_liftover_generic_wave  one wavefront per hit the streaming kernel declines: three passes over the record's
//                       ops (boundaries, merge of adjacent runs through LDS, emission).  It takes every case the streaming kernel declines
//                       (irregular CIGARs: N/S/H/P, zero lengths, adjacent ops of one type that must
//                       merge (paf.rs:602-620); the legacy binary-search policy when the duplicate
//                       choice matters; look-aheads / look-backs longer than RB_WALK_MAX ops).
//
// Roofline: HBM.  Algorithmic bytes: 4 B per input op + 48 B per record + 88 B per hit + 4 B per
// emitted op.  No MFMA: integer / index work only.
#include "rb_lift.h"
#include "rb_launch.h"
#include <type_traits>
#include <algorithm>

__global__ __launch_bounds__(256) void rb_k_count_hits(rb_lift_params p) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= p.n_rec) return;
    uint64_t cnt = 0;
    const rb_norm_row *nr = &p.norm[r];
    const uint32_t c = p.contig[r];
    if (nr->status == RB_ST_OK && c < p.n_contig) {
        const uint64_t ws = p.cw_off[c], we = p.cw_off[c + 1];
        const uint64_t t_st = nr->t_st, t_en = nr->t_en;
        if (p.cw_mono[c]) {
            const uint64_t lo = rb_lower_en_gt(p.w_en, ws, we, t_st);
            const uint64_t hi = rb_lower_st_ge(p.w_st, ws, we, t_en);
            cnt = hi > lo ? hi - lo : 0;
            p.win_lo[r] = (uint32_t)lo;
        } else {
            for (uint64_t i = ws; i < we; i++) cnt += (t_en > p.w_st[i] && t_st < p.w_en[i]) ? 1 : 0;
        }
    }
    p.hit_off[p.canon_pos[r]] = cnt;
}

// ------------------------------------------------------------------------------------------------
// exclusive scan of u64 counts, in place, n + 1 outputs (3 small launches)
// ------------------------------------------------------------------------------------------------
#define RB_SCAN_PER_BLOCK 2048
__global__ __launch_bounds__(256) void rb_k_scan_partial(const uint64_t *v, uint64_t n, uint64_t *block_sums) {
    __shared__ uint64_t sh[4];
    const uint64_t base = (uint64_t)blockIdx.x * RB_SCAN_PER_BLOCK;
    uint64_t s = 0;
    for (int k = 0; k < RB_SCAN_PER_BLOCK / 256; k++) {
        uint64_t i = base + (uint64_t)k * 256 + threadIdx.x;
        if (i < n) s += v[i];
    }
    s = rb_wave_sum_u64(s);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) block_sums[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}
__global__ __launch_bounds__(256) void rb_k_scan_top(uint64_t *block_sums, uint64_t n_blocks) {
    // single block: serial over chunks of 256 (n_blocks is a few thousand at most)
    __shared__ uint64_t sh[256];
    __shared__ uint64_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (uint64_t b = 0; b < n_blocks; b += 256) {
        uint64_t i = b + threadIdx.x;
        uint64_t x = i < n_blocks ? block_sums[i] : 0;
        sh[threadIdx.x] = x;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            uint64_t y = threadIdx.x >= (unsigned)off ? sh[threadIdx.x - off] : 0;
            __syncthreads();
            sh[threadIdx.x] += y;
            __syncthreads();
        }
        uint64_t incl = sh[threadIdx.x];
        if (i < n_blocks) block_sums[i] = carry + incl - x;
        __syncthreads();
        if (threadIdx.x == 255) carry += incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) block_sums[n_blocks] = carry;
}
__global__ __launch_bounds__(256) void rb_k_scan_apply(uint64_t *v, uint64_t n, const uint64_t *block_sums, uint64_t *total_out) {
    __shared__ uint64_t sh[256];
    const uint64_t base = (uint64_t)blockIdx.x * RB_SCAN_PER_BLOCK;
    // each thread owns 8 consecutive elements
    uint64_t x[RB_SCAN_PER_BLOCK / 256];
    uint64_t s = 0;
    const uint64_t i0 = base + (uint64_t)threadIdx.x * (RB_SCAN_PER_BLOCK / 256);
#pragma unroll
    for (int k = 0; k < RB_SCAN_PER_BLOCK / 256; k++) {
        x[k] = (i0 + k < n) ? v[i0 + k] : 0;
        s += x[k];
    }
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        uint64_t y = threadIdx.x >= (unsigned)off ? sh[threadIdx.x - off] : 0;
        __syncthreads();
        sh[threadIdx.x] += y;
        __syncthreads();
    }
    uint64_t run = block_sums[blockIdx.x] + sh[threadIdx.x] - s;
#pragma unroll
    for (int k = 0; k < RB_SCAN_PER_BLOCK / 256; k++) {
        if (i0 + k < n) v[i0 + k] = run;
        run += x[k];
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 255) {
        const uint64_t total = block_sums[gridDim.x];
        v[n] = total;
        if (total_out) *total_out = total;
    }
}

// ------------------------------------------------------------------------------------------------
// clip jobs: what a wave needs about its record, gathered into the record's schedule slot
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rb_k_make_jobs(rb_lift_params p) {
    // one thread per RECORD (rows, offsets and hit counts are read in memory order), the job goes to the record's slot
    const uint64_t r64 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r64 >= p.n_rec) return;
    const uint32_t r = (uint32_t)r64;
    const uint64_t w = p.slot_of[r];
    const rb_norm_row *nr = &p.norm[r];
    rb_job j;
    j.r = r;
    j.n = nr->n_ops;
    j.rec0 = p.op_off[r] + nr->first_op;
    j.t_st = nr->t_st, j.t_en = nr->t_en, j.q_st = nr->q_st, j.q_en = nr->q_en;
    const uint64_t k = p.canon_pos[r];
    const bool brk = p.brk_mode != 0; // one-walk break-paf: the pieces are not known yet (one pass per record, rows placed afterwards)
    const uint64_t h0 = brk ? 0ull : p.hit_off[k], nh = brk ? 1ull : p.hit_off[k + 1] - h0;
    const bool explicit_w = brk || p.x_st != nullptr;
    const uint32_t cg = p.contig[r];
    const bool mono = explicit_w || (cg < p.n_contig && p.cw_mono[cg] != 0);
    uint32_t f = 0;
    const bool provisional = (nr->flags & RB_F_PROVISIONAL) != 0; // fused scan: the clip kernel verifies the record itself,
    if (nr->status == RB_ST_OK && (nh != 0 || provisional)) {     // also when no window overlaps it (liftover.rs:119-121)
        if (h0 + nh > p.rows_cap) f |= RB_JOB_ROWS_OVERFLOW;
        else f |= RB_JOB_VALID;
    }
    if ((nr->flags & RB_F_REGULAR) || (provisional && !(nr->flags & RB_F_ENDS_NOT_MATCH))) f |= RB_JOB_REGULAR;
    if (p.strand[r] == (uint8_t)'-') f |= RB_JOB_MINUS;
    if (mono) f |= RB_JOB_MONO;
    j.flags = f;
    j.h0 = (uint32_t)h0;
    j.nh = (uint32_t)nh;
    j.lo = (explicit_w || !mono || !(f & RB_JOB_VALID) || nh == 0) ? 0u : p.win_lo[r];
    p.jobs[w] = j;
}

// ------------------------------------------------------------------------------------------------
// streaming kernel: the body is rb_stream.h, with the load ring at v88..v103 (k_liftover_list.hip: the same body over a list of
// records, the same ring)
// ------------------------------------------------------------------------------------------------
#define RB_RING_BASE 88
#define RB_RING_TOP_N 103
#define RB_SPILL_ROOM 4
#define RB_WPE 4, 5
#include "rb_stream.h"
// the builds of the kernel (an attribute cannot depend on a template parameter): liftover and its diagnostics build; break-paf in one
// walk, which captures nothing and keeps the ring at v80 and five waves per SIMD, is k_liftover_brk.hip
#define RB_STREAM_KERNEL(NAME, BRK, DIAG, ROOM)                                                                                   \
    __global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RB_WPE), amdgpu_num_vgpr(RB_RING_BASE - (ROOM)))) void NAME(rb_lift_params p_) { \
        (void)p_; /* (read through the kernel-argument segment, see the top of rb_stream_record) */                                \
        rb_stream_record<BRK, DIAG>();                                                                                            \
    }
RB_STREAM_KERNEL(rb_k_liftover_stream, false, false, RB_SPILL_ROOM)
RB_STREAM_KERNEL(rb_k_liftover_stream_diag, false, true, 5)
// (no diagnostics build of the break form: its spilled scalar registers land in the ring -- tools/check_ring.py --, and nothing asks for it)

// ------------------------------------------------------------------------------------------------
// clips that found no place of their own in a slot (windows overlapping deeper than the slots, window lists that are
// not sorted, no room for slots in out_ops): one wavefront per clip copies it into the arena area
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rb_k_copy_clips(rb_lift_params p) {
    const uint64_t n_copy = *p.copy_count;
    const int lane = rb_lane();
    for (uint64_t e = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); e < n_copy; e += (uint64_t)gridDim.x * 4u) {
        const uint4 d = p.copy_list[e]; // row, first kept op (of the normalised record), clipped first / last length (0: keep)
        rb_hit_row *row = &p.rows[d.x];
        const uint32_t rec = row->rec, n = row->out_n;
        const uint32_t *src = p.ops + p.op_off[rec] + p.norm[rec].first_op + d.y;
        const uint32_t padded = (n + 3u) & ~3u;
        const uint32_t arena = (uint32_t)(e % p.n_arena);
        unsigned long long b0 = 0;
        if (lane == 0) b0 = atomicAdd(&p.arena_cur[(uint64_t)arena * RB_ARENA_STRIDE], (unsigned long long)padded);
        b0 = rb_first64(b0);
        if (b0 + padded > p.arena_size) {
            if (lane == 0) p.counters->overflow = 1;
            continue;
        }
        const uint64_t off = p.arena_origin + (uint64_t)arena * p.arena_size + b0;
        uint32_t *dst = p.out_ops + off;
        for (uint32_t k = (uint32_t)lane; k < n; k += 64u) {
            uint32_t w = src[k];
            const uint32_t len0 = rb_len(w);
            uint32_t len = len0;
            if (n == 1u && d.z && d.w) len = d.z + d.w - len0;
            else {
                if (k == 0 && d.z) len = d.z;
                if (k == n - 1u && d.w) len = d.w;
            }
            dst[k] = (len << 4) | rb_opc(w);
        }
        if (lane == 0) row->out_off = off;
    }
}

// ------------------------------------------------------------------------------------------------
// generic hit, one thread, serial, fully general (unit semantics evaluated in op space): what the wave kernel below hands unsorted arrays to
// ------------------------------------------------------------------------------------------------
struct rb_gwalk {
    const uint32_t *ops;
    uint32_t n;
};

// legacy Rust binary_search (1.52..1.81) on a virtual array whose equal range is [klo, khi]
__device__ uint64_t rb_legacy_probe(uint64_t N, uint64_t klo, uint64_t khi) {
    uint64_t size = N, left = 0, right = N;
    while (left < right) {
        const uint64_t mid = left + size / 2;
        if (mid < klo)
            left = mid + 1;
        else if (mid > khi)
            right = mid;
        else
            return mid;
        size = right - left;
    }
    return klo;
}

// tpos_aln of a record whose target start is 0 and whose first ops consume no reference begins with units at
// t_pos = -1, i.e. u64::MAX (paf.rs:505, :531): the array is then NOT sorted and slice::binary_search returns whatever
// its probe sequence leads to.  This reproduces that probe sequence on the virtual array (value of a unit = walk of the
// ops), for both generations of the Rust standard library.  Returns true and the index on Ok, false on Err.
__device__ uint64_t rb_unit_tpos(const uint32_t *ops, uint32_t n, uint64_t t_st, uint64_t unit) {
    int64_t tpos = (int64_t)t_st - 1;
    uint64_t U = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t opc = rb_wopc(ops, i), len = rb_wlen(ops, i);
        const bool isref = opc <= 8 && rb_in(RB_REF_MASK, opc);
        if (unit < U + len) return (uint64_t)(isref ? tpos + (int64_t)(unit - U) + 1 : tpos); // (-1 wraps to u64::MAX)
        U += len;
        if (isref) tpos += len;
    }
    return ~0ull;
}
__device__ bool rb_bsearch_units(const uint32_t *ops, uint32_t n, uint64_t t_st, uint64_t N, uint64_t key, int policy, uint64_t *idx) {
    auto cmp = [&](uint64_t mid) -> int {
        const uint64_t v = rb_unit_tpos(ops, n, t_st, mid);
        return v < key ? -1 : (v > key ? 1 : 0);
    };
    if (policy != RB_BSEARCH_LEGACY) { // rustc >= 1.82
        uint64_t size = N;
        if (size == 0) return false;
        uint64_t base = 0;
        while (size > 1) {
            const uint64_t half = size / 2, mid = base + half;
            base = cmp(mid) > 0 ? base : mid;
            size -= half;
        }
        *idx = base;
        return cmp(base) == 0;
    }
    uint64_t size = N, left = 0, right = N; // 1.52 .. 1.81
    while (left < right) {
        const uint64_t mid = left + size / 2;
        const int c = cmp(mid);
        if (c < 0) left = mid + 1;
        else if (c > 0) right = mid;
        else {
            *idx = mid;
            return true;
        }
        size = right - left;
    }
    return false;
}

// one hit, one thread, serial (the general case of the general case)
__device__ void rb_generic_serial_hit(const rb_lift_params &p, const uint64_t g) {
    for (int once = 0; once < 1; once++) {
        const uint64_t hrow = p.gen_list[g];
        rb_hit_row *row = &p.rows[hrow];
        const uint32_t r = row->rec, win = row->win;
        const rb_norm_row *nr = &p.norm[r];
        if (nr->status != RB_ST_OK) { // fused scan: the record was handed back and the full scan found the reference would panic on it
            row->status = (uint16_t)nr->status;
            row->out_n = 0;
            row->out_off = 0;
            row->t_st = row->t_en = row->q_st = row->q_en = 0;
            row->nmatch = row->aln_len = 0;
            continue;
        }
        const uint64_t t_st = nr->t_st, t_en = nr->t_en, q_st = nr->q_st, q_en = nr->q_en;
        const bool minus = p.strand[r] == (uint8_t)'-';
        const uint32_t n = nr->n_ops;
        const uint32_t *ops = p.ops + p.op_off[r] + nr->first_op;
        const uint64_t wst = p.x_st ? p.x_st[hrow] : p.wo_st[win];
        const uint64_t wen = p.x_en ? p.x_en[hrow] : p.wo_en[win];
        rb_hit_row w;
        w.rec = r;
        w.win = win;
        w.flags = RB_HIT_GENERIC;
        w.status = RB_ST_OK;
        w.out_n = 0;
        w.out_off = 0;
        w.t_st = w.t_en = w.q_st = w.q_en = 0;
        w.nmatch = w.aln_len = 0;
        const uint32_t arena = (uint32_t)(g % p.n_arena);

        if (t_st > wst && t_en < wen) { // liftover.rs:23-25: verbatim clone, own id
            w.flags |= RB_HIT_INSIDE;
            w.t_st = t_st;
            w.t_en = t_en;
            w.q_st = q_st;
            w.q_en = q_en;
            w.nmatch = nr->nmatch;
            w.aln_len = nr->aln_len;
            w.out_n = n;
            const uint32_t padded = (n + 3u) & ~3u;
            const unsigned long long b0 = atomicAdd(&p.arena_cur[(uint64_t)arena * RB_ARENA_STRIDE], (unsigned long long)padded);
            if (b0 + padded <= p.arena_size) {
                w.out_off = p.arena_origin + (uint64_t)arena * p.arena_size + b0;
                for (uint32_t i = 0; i < n; i++) p.out_ops[w.out_off + i] = ops[i];
            } else {
                p.counters->overflow = 1;
            }
            *row = w;
            continue;
        }
        // positions to look up (liftover.rs:28, :38-40)
        const int64_t ps = (int64_t)(wst > t_st ? wst : t_st);
        const int64_t pe = (int64_t)(wen < t_en ? wen : t_en) - 1;
        // pass 1: equal ranges of ps and pe in the virtual tpos_aln, total units (paf.rs:505-534)
        uint64_t N = 0;
        uint64_t s_lo = 0, s_hi = 0, e_lo = 0, e_hi = 0;
        bool s_found = false, e_found = false;
        {
            int64_t tpos = (int64_t)t_st - 1;
            for (uint32_t i = 0; i < n; i++) {
                const uint32_t opc = rb_wopc(ops, i), len = rb_wlen(ops, i);
                if (len == 0) continue;
                if (opc <= 8 && rb_in(RB_REF_MASK, opc)) {
                    // units N..N+len-1 hold tpos+1 .. tpos+len
                    if (ps > tpos && ps <= tpos + (int64_t)len) {
                        const uint64_t u = N + (uint64_t)(ps - tpos - 1);
                        if (!s_found) { s_found = true; s_lo = u; }
                        s_hi = u;
                    }
                    if (pe > tpos && pe <= tpos + (int64_t)len) {
                        const uint64_t u = N + (uint64_t)(pe - tpos - 1);
                        if (!e_found) { e_found = true; e_lo = u; }
                        e_hi = u;
                    }
                    tpos += len;
                } else {
                    if (ps == tpos && tpos >= 0) {
                        if (!s_found) { s_found = true; s_lo = N; }
                        s_hi = N + len - 1;
                    }
                    if (pe == tpos && tpos >= 0) {
                        if (!e_found) { e_found = true; e_lo = N; }
                        e_hi = N + len - 1;
                    }
                }
                N += len;
            }
        }
        // units at t_pos = -1 in front of the first reference-consuming op (only possible with t_st == 0): the array is not
        // sorted, so the equal ranges do not tell what binary_search returns; its probe sequence is replayed instead
        bool wrapped = false;
        if (t_st == 0)
            for (uint32_t i = 0; i < n; i++) {
                if (rb_wlen(ops, i) == 0) continue; // (a zero-length op adds no unit)
                const uint32_t opc = rb_wopc(ops, i);
                wrapped = !(opc <= 8 && rb_in(RB_REF_MASK, opc));
                break;
            }
        uint64_t ks, ke;
        if (wrapped) {
            if (!rb_bsearch_units(ops, n, t_st, N, (uint64_t)ps, p.policy, &ks) || !rb_bsearch_units(ops, n, t_st, N, (uint64_t)pe, p.policy, &ke)) {
                w.status = RB_ST_PANIC_NOTFOUND;
                *row = w;
                continue;
            }
        } else {
            if (!s_found || !e_found) { // binary_search Err -> panic (liftover.rs:31, :42)
                w.status = RB_ST_PANIC_NOTFOUND;
                *row = w;
                continue;
            }
            ks = p.policy == RB_BSEARCH_LEGACY ? rb_legacy_probe(N, s_lo, s_hi) : s_hi;
            ke = p.policy == RB_BSEARCH_LEGACY ? rb_legacy_probe(N, e_lo, e_hi) : e_hi;
        }
        // pass 2: a = first match-type unit >= ks (else N); b = last match-type unit <= ke (else 0)
        uint64_t a = N, b = 0;
        uint64_t Ra = 0, Qa = 0, Ma = 0, nRb = 0, nQb = 0, nMb = 0;
        {
            uint64_t U = 0, R = 0, Q = 0, M = 0;
            bool a_set = false;
            for (uint32_t i = 0; i < n; i++) {
                const uint32_t opc = rb_wopc(ops, i), len = rb_wlen(ops, i);
                if (len == 0) continue;
                const bool isref = opc <= 8 && rb_in(RB_REF_MASK, opc), isq = opc <= 8 && rb_in(RB_QRY_MASK, opc);
                const bool ism = opc <= 8 && rb_in(RB_MATCH_MASK, opc);
                if (ism) {
                    if (!a_set && U + len > ks) {
                        a = ks > U ? ks : U;
                        const uint64_t off = a - U;
                        Ra = R + off;
                        Qa = Q + off;
                        Ma = M + off;
                        a_set = true;
                    }
                    if (U <= ke) {
                        b = (U + len - 1) < ke ? (U + len - 1) : ke;
                        const uint64_t off = b - U;
                        nRb = R + off + 1;
                        nQb = Q + off + 1;
                        nMb = M + off + 1;
                    }
                }
                U += len;
                if (isref) R += len;
                if (isq) Q += len;
                if (ism) M += len;
            }
        }
        if (a > b || a >= N) { // liftover.rs:52-54
            w.status = RB_ST_NONE_INDEL;
            *row = w;
            continue;
        }
        // pass 3: count run-length-merged ops of units [a, b] (paf.rs:602-620)
        uint32_t out_n = 0; // (in words: a merged run of 2^28 bases and more takes two)
        {
            uint64_t U = 0;
            uint32_t prev = RB_NULL_OP, run = 0;
            for (uint32_t i = 0; i < n; i++) {
                const uint32_t opc = rb_wopc(ops, i), len = rb_wlen(ops, i);
                if (len == 0) continue;
                const uint64_t u0 = U, u1 = U + len - 1;
                U += len;
                if (u1 < a) continue;
                if (u0 > b) break;
                const uint64_t c0 = u0 > a ? u0 : a, c1 = u1 < b ? u1 : b;
                if (opc != prev) {
                    if (prev != RB_NULL_OP) out_n += 1u + ((run >> RB_LEN_BITS_WORD) ? 1u : 0u);
                    run = 0;
                }
                run += (uint32_t)(c1 - c0 + 1);
                prev = opc;
            }
            if (prev != RB_NULL_OP) out_n += 1u + ((run >> RB_LEN_BITS_WORD) ? 1u : 0u);
        }
        w.t_st = t_st + Ra; // liftover.rs:57-60, :77-82 (a and b are match-type units)
        w.t_en = t_st + nRb;
        if (!minus) {
            w.q_st = q_st + Qa;
            w.q_en = q_st + nQb;
        } else {
            w.q_st = q_en - nQb;
            w.q_en = q_en - Qa;
        }
        w.nmatch = (uint32_t)(nMb - Ma);
        w.aln_len = (uint32_t)(b - a + 1);
        w.out_n = out_n;
        const uint32_t padded = (out_n + 3u) & ~3u;
        const unsigned long long b0 = atomicAdd(&p.arena_cur[(uint64_t)arena * RB_ARENA_STRIDE], (unsigned long long)padded);
        if (b0 + padded > p.arena_size) {
            p.counters->overflow = 1;
            *row = w;
            continue;
        }
        w.out_off = p.arena_origin + (uint64_t)arena * p.arena_size + b0;
        { // pass 4: emit
            uint64_t U = 0;
            uint32_t prev = RB_NULL_OP, run = 0;
            uint64_t o = w.out_off;
            for (uint32_t i = 0; i < n; i++) {
                const uint32_t opc = rb_wopc(ops, i), len = rb_wlen(ops, i);
                if (len == 0) continue;
                const uint64_t u0 = U, u1 = U + len - 1;
                U += len;
                if (u1 < a) continue;
                if (u0 > b) break;
                const uint64_t c0 = u0 > a ? u0 : a, c1 = u1 < b ? u1 : b;
                const uint32_t piece = (uint32_t)(c1 - c0 + 1);
                if (opc != prev) {
                    if (prev != RB_NULL_OP) o += rb_emit_run(p.out_ops + o, run, prev);
                    prev = opc;
                    run = piece;
                } else {
                    run += piece;
                }
            }
            if (prev != RB_NULL_OP) o += rb_emit_run(p.out_ops + o, run, prev);
        }
        *row = w;
    }
}

// ------------------------------------------------------------------------------------------------
// generic kernel, one WAVEFRONT per hit: the same unit semantics, every walk of the ops a pass of 64 ops per step with wave scans.
//   pass 1  equal ranges of the window's first / last base in the virtual tpos_aln (paf.rs:505-534) and the number of units
//   pass 2  first match-type unit >= the start index, last one <= the end index (paf.rs:551-558), with the prefixes there
//   pass 3  the ops between them, first / last length cut, adjacent ops of one type merged (paf.rs:602-620), zero lengths dropped
// A tpos_aln that is not sorted (units at position -1, see rb_bsearch_units) goes to the serial code above.
// ------------------------------------------------------------------------------------------------
// Checkpoints for the generic kernel (rb_lift_params::gen_cp): one wavefront per entry of the generic list walks the entry's record
// once and leaves, before every RB_GCP-th kept op, the units / reference / query / match bases so far.  The hits of a record follow
// each other in the list: only the first of a run builds (a record that appears in two runs is built twice, with the same values).
__device__ __forceinline__ uint4 *rb_gen_cp_of(const rb_lift_params &p, uint32_t r, uint32_t first_op) {
    return p.gen_cp + ((p.op_off[r] + first_op) / RB_GCP + r);
}
__global__ __launch_bounds__(256) void rb_k_generic_checkpoints(rb_lift_params p) {
    static_assert(RB_GCP == 64u, "one 16-byte load per lane covers four checkpoint intervals: lanes 0, 16, 32, 48 stand at their starts");
    const uint32_t wib = threadIdx.x >> 6;
    const int lane = rb_lane();
    const uint64_t n_gen = p.counters->n_generic;
    for (uint64_t g = (uint64_t)blockIdx.x * 4u + wib; g < n_gen; g += (uint64_t)gridDim.x * 4u) {
        const uint32_t r = p.rows[p.gen_list[g]].rec;
        if (g > 0 && p.rows[p.gen_list[g - 1]].rec == r) continue;
        const rb_norm_row *nr = &p.norm[r];
        if (nr->status != RB_ST_OK) continue;
        const uint32_t n = nr->n_ops;
        if (n <= RB_GCP) continue; // (one checkpoint, the record's start: nothing to look up)
        const uint32_t *ops = p.ops + p.op_off[r] + nr->first_op;
        uint4 *cp = rb_gen_cp_of(p, r, nr->first_op);
        auto load = [&](uint32_t c0) -> uint4 { // my four ops of the 256 that start at c0 (past the record: zero-length M ops)
            const uint32_t i = c0 + 4u * (uint32_t)lane;
            if (i + 3u < n) return rb_load4_unaligned(ops + i);
            return make_uint4(i < n ? ops[i] : 0u, i + 1u < n ? ops[i + 1u] : 0u, i + 2u < n ? ops[i + 2u] : 0u, 0u);
        };
        // The fields are 32 bits wide.  A record whose units in front of a checkpoint reach 2^32 (continuation words: up to 15 * 2^28
        // bases a word) gets none: checkpoint 0 -- zeros otherwise -- says so, and rb_k_liftover_generic_wave walks such a record
        // from its first op with its own 64-bit sums, as it does without checkpoints.
        // Round 5: a checkpoint every 64 ops (256 before): a walk of the wave kernel starts in the step that holds what it looks for
        // instead of up to three steps in front of it -- the kernel is bound by the instructions of its steps.  A lane sums its four
        // ops, wave scans give every lane the sums in front of it, and the lanes that stand at a multiple of 64 ops write.
        uint64_t U = 0;
        uint32_t R = 0, Q = 0, M = 0;
        uint4 nxt = load(0u);
        for (uint32_t c0 = 0; c0 < n; c0 += 256u) {
            const uint4 cur = nxt;
            if (c0 + 256u < n) nxt = load(c0 + 256u); // (in flight while these ops are summed)
            const uint32_t w4[4] = {cur.x, cur.y, cur.z, cur.w};
            uint64_t u = 0; // (the reference / query / match sums are parts of it: they stay below 2^32 wherever a checkpoint is written)
            uint32_t rr = 0, q = 0, m = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t i = c0 + 4u * (uint32_t)lane + (uint32_t)k;
                uint32_t opc = rb_opc(w4[k]), len = rb_len(w4[k]);
                if (opc == RB_OP_CONT && i < n) opc = rb_wopc(ops, i), len = rb_wlen(ops, i);
                const bool okc = opc <= 8u;
                u += len;
                rr += okc && rb_in(RB_REF_MASK, opc) ? len : 0u;
                q += okc && rb_in(RB_QRY_MASK, opc) ? len : 0u;
                m += okc && rb_in(RB_MATCH_MASK, opc) ? len : 0u;
            }
            // (u < 2^34 a lane: scanned as its low 24 bits and what is above them, neither of which can leave 32 bits over 64 lanes)
            const uint64_t iu = (uint64_t)rb_wave_scan_incl((uint32_t)u & 0xFFFFFFu) + ((uint64_t)rb_wave_scan_incl((uint32_t)(u >> 24)) << 24);
            const uint32_t ir = rb_wave_scan_incl(rr), iq = rb_wave_scan_incl(q), im = rb_wave_scan_incl(m);
            const bool mine = (lane & 15) == 0 && c0 + 4u * (uint32_t)lane < n; // a checkpoint stands in front of my first op
            const uint64_t Uv = U + iu - u;
            if (__ballot(mine && (Uv >> 32)) != 0ull) {
                if (lane == 0) cp[0] = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
                break;
            }
            if (mine) cp[c0 / RB_GCP + ((uint32_t)lane >> 4)] = make_uint4((uint32_t)Uv, R + ir - rr, Q + iq - q, M + im - m);
            U += rb_readlane<uint64_t>(iu, 63), R += rb_readlane<uint32_t>(ir, 63), Q += rb_readlane<uint32_t>(iq, 63), M += rb_readlane<uint32_t>(im, 63);
        }
    }
}
__device__ __forceinline__ uint64_t rb_wave_min_u64(uint64_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t o = __shfl_xor(v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ uint64_t rb_wave_max_u64(uint64_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}
// One thread per generic hit: everything the wave kernel needs to start on it, gathered -- the dependent chain list entry -> row -> record's
// row, offsets, strand -> windows -> checkpoint searches is walked here by as many threads as there are hits, not by a wave per hit in front
// of its first op (round 5; the stream kernel got its rb_job the same way in round 1).
__global__ __launch_bounds__(256) void rb_k_generic_jobs(rb_lift_params p) {
    const uint64_t n_gen = p.counters->n_generic;
    for (uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x; g < n_gen; g += (uint64_t)gridDim.x * 256u) {
        const uint32_t hrow = p.gen_list[g];
        const rb_hit_row *row = &p.rows[hrow];
        const uint32_t r = row->rec, win = row->win;
        const rb_norm_row *nr = &p.norm[r];
        rb_gja A;
        A.t_st = nr->t_st, A.t_en = nr->t_en, A.q_st = nr->q_st, A.q_en = nr->q_en;
        A.n = nr->n_ops;
        A.ops_off = p.op_off[r] + nr->first_op;
        A.wst = p.x_st ? p.x_st[hrow] : p.wo_st[win];
        A.wen = p.x_en ? p.x_en[hrow] : p.wo_en[win];
        A.k2 = 0;
        uint32_t k1 = 0, has_cp = 0;
        const uint32_t status = nr->status;
        if (status == RB_ST_OK && !(A.t_st > A.wst && A.t_en < A.wen)) {
            const uint4 *gcp = (p.gen_cp && A.n > RB_GCP) ? rb_gen_cp_of(p, r, nr->first_op) : nullptr;
            if (gcp && gcp[0].x == 0xFFFFFFFFu) gcp = nullptr; // (a record of 2^32 units and more has no checkpoints)
            if (gcp) {
                has_cp = 1;
                const uint32_t ncp = (A.n + RB_GCP - 1u) / RB_GCP;
                auto last_le = [&](uint64_t target) -> uint32_t { // the last checkpoint with at most `target` reference bases in front of it (checkpoint 0 holds zeros)
                    uint32_t lo = 0, hi = ncp;
                    while (hi - lo > 1u) {
                        const uint32_t mid = (lo + hi) >> 1;
                        if ((uint64_t)gcp[mid].y <= target) lo = mid; else hi = mid;
                    }
                    return lo;
                };
                const int64_t ps = (int64_t)(A.wst > A.t_st ? A.wst : A.t_st), pe = (int64_t)(A.wen < A.t_en ? A.wen : A.t_en) - 1;
                k1 = last_le((uint64_t)ps - A.t_st);
                const uint32_t k2 = pe >= ps ? last_le((uint64_t)pe - A.t_st) : 0u;
                if (k2 > k1 + 1u) A.k2 = k2;
            }
        }
        p.gj_a[g] = A;
        p.gj_b[g] = make_uint4(hrow, r, win, (status << 16) | (((uint32_t)row->flags & 0xFFu) << 8) | (has_cp << 1) | (p.strand[r] == (uint8_t)'-' ? 1u : 0u));
        p.gj_c[g] = make_uint2(nr->aln_len, k1);
    }
}
#define RB_GW_WPE 4 // (round 5: the kernel wants 127 registers; at five waves per SIMD (96) it spilled 74 of them to scratch, at four it spills none:
                    //  11.58 -> 10.48 ms on the irregular workload, and two, three or four waves take the same time -- the kernel is bound by the
                    //  instructions it issues, not by what it waits for.  tools/r05_gw_ab.sh, same box.  Earlier in the round, with groups of
                    //  four steps: 5 waves 12.5 ms, 6 waves 16.8, 8 waves 17.0 -- against 15.0 for the round-3 form at 8 waves)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RB_GW_WPE))) void rb_k_liftover_generic_wave(rb_lift_params p) {
    __shared__ uint32_t run_tot_all[4][64], run_opc_all[4][64];
    const uint32_t wib = threadIdx.x >> 6;
    uint32_t *run_tot = run_tot_all[wib], *run_opc = run_opc_all[wib];
    const int lane = rb_lane();
    const uint64_t n_gen = p.counters->n_generic;
    for (uint64_t g = (uint64_t)blockIdx.x * 4u + wib; g < n_gen; g += (uint64_t)gridDim.x * 4u) {
        // the hit's descriptor (rb_k_generic_jobs): three loads at addresses the whole wave shares, one trip
        const rb_gja A_ = p.gj_a[g];
        const uint4 B_ = p.gj_b[g];
        const uint2 C_ = p.gj_c[g];
        const uint64_t hrow = rb_first(B_.x);
        const uint32_t r = rb_first(B_.y), win = rb_first(B_.z), gfl = rb_first(B_.w);
        rb_hit_row *row = &p.rows[hrow];
        rb_hit_row w;
        w.rec = r;
        w.win = win;
        w.flags = RB_HIT_GENERIC;
        w.status = RB_ST_OK;
        w.out_n = 0;
        w.out_off = 0;
        w.t_st = w.t_en = w.q_st = w.q_en = 0;
        w.nmatch = w.aln_len = 0;
        if ((gfl >> 16) != RB_ST_OK) { // fused scan: the record was handed back and the full scan found the reference would panic on it
            w.status = (uint16_t)(gfl >> 16);
            w.flags = (uint16_t)((gfl >> 8) & 0xFFu);
            if (lane == 0) *row = w;
            continue;
        }
        const uint64_t t_st = rb_first64(A_.t_st), t_en = rb_first64(A_.t_en), q_st = rb_first64(A_.q_st), q_en = rb_first64(A_.q_en);
        const bool minus = (gfl & 1u) != 0u;
        const uint32_t n = rb_first(A_.n);
        const uint64_t ops_off = rb_first64(A_.ops_off);
        const uint32_t *ops = p.ops + ops_off;
        const uint64_t wst = rb_first64(A_.wst), wen = rb_first64(A_.wen);
        const uint32_t rec_units = rb_first(C_.x);
        const uint32_t arena = (uint32_t)(g % p.n_arena);
        auto reserve = [&](uint32_t padded, uint64_t *off) -> bool { // room in an arena, for the whole wave
            unsigned long long b0 = 0;
            if (lane == 0) b0 = atomicAdd(&p.arena_cur[(uint64_t)arena * RB_ARENA_STRIDE], (unsigned long long)padded);
            b0 = rb_first64(b0);
            if (b0 + padded > p.arena_size) {
                if (lane == 0) p.counters->overflow = 1;
                return false;
            }
            *off = p.arena_origin + (uint64_t)arena * p.arena_size + b0;
            return true;
        };
        if (t_st > wst && t_en < wen) { // liftover.rs:23-25: verbatim clone, own id
            w.flags |= RB_HIT_INSIDE;
            w.t_st = t_st, w.t_en = t_en, w.q_st = q_st, w.q_en = q_en;
            w.nmatch = p.norm[r].nmatch, w.aln_len = rec_units;
            w.out_n = n;
            uint64_t off;
            if (reserve((n + 3u) & ~3u, &off)) {
                w.out_off = off;
                for (uint32_t i = (uint32_t)lane; i < n; i += 64u) p.out_ops[off + i] = ops[i];
            }
            if (lane == 0) *row = w;
            continue;
        }
        const int64_t ps = (int64_t)(wst > t_st ? wst : t_st); // positions to look up (liftover.rs:28, :38-40)
        const int64_t pe = (int64_t)(wen < t_en ? wen : t_en) - 1;
        // ---- where the walks start: the last checkpoint with at most ps - t_st reference bases in front of it (every unit at
        //      position ps, and everything behind it, lies at or behind that op).  The question pass 1 answers with the record's
        //      first ops -- do units at position -1 come first? -- is asked of them directly then. ----
        uint32_t c_start = 0, c_end1 = 0;               // c_end1: where the walk for the window's END may resume (pass 1)
        uint4 cp0 = make_uint4(0u, 0u, 0u, 0u), cp_e1 = cp0;
        bool first_seen = false, wrapped = false;
        const uint4 *gcp = (gfl & 2u) ? p.gen_cp + (ops_off / RB_GCP + r) : nullptr; // (rb_gen_cp_of; rb_k_generic_jobs has looked: there are checkpoints)
        const uint32_t ncp = (n + RB_GCP - 1u) / RB_GCP;
        // the last checkpoint whose field (1: reference bases, 0: units) is <= target (checkpoint 0 holds zeros); the fields never decrease
        auto cp_search = [&](int field, uint64_t target) -> uint32_t {
            uint32_t k1 = 0;
            for (uint32_t kb = 0; kb < ncp; kb += 64u) {
                const uint32_t k = kb + (uint32_t)lane;
                const uint4 c = gcp[k < ncp ? k : 0u];
                const uint64_t m = __ballot(k < ncp && (uint64_t)(field ? c.y : c.x) <= target);
                if (!m) break;
                k1 = kb + (uint32_t)__builtin_popcountll(m) - 1u; // (m is a run of low bits)
                if (m != ~0ull) break;
            }
            return k1;
        };
        if (gcp) {
            const uint32_t k1 = rb_first(C_.y), k2 = rb_first(A_.k2); // (searched by rb_k_generic_jobs: k2 != 0 means k2 > k1 + 1)
            if (k2) c_end1 = k2 * RB_GCP, cp_e1 = gcp[k2];
            if (k1) {
                c_start = k1 * RB_GCP;
                cp0 = gcp[k1];
                if (t_st == 0) { // (only then can a unit sit at position -1)
                    for (uint32_t c0 = 0; c0 < n && !first_seen; c0 += 64u) {
                        const uint32_t i = c0 + (uint32_t)lane;
                        uint32_t opc = RB_NULL_OP, len = 0u;
                        if (i < n) opc = rb_wopc(ops, i), len = rb_wlen(ops, i);
                        const uint64_t m = __ballot(len != 0u);
                        if (m) {
                            first_seen = true;
                            wrapped = !((__ballot(opc <= 8u && rb_in(RB_REF_MASK, opc)) >> __builtin_ctzll(m)) & 1ull);
                        }
                    }
                }
                first_seen = true;
            }
        }
        // ---- pass 1 ----
        uint64_t s_lo = ~0ull, s_hi = 0, e_lo = ~0ull, e_hi = 0;
        uint64_t Ub = cp0.x, Rb = cp0.y;
        // (the next step's ops are asked for before this step's are looked at: a hit is a chain of dependent steps, and the load is the
        //  longest link of each)
        auto ld = [&](uint32_t c0_) -> uint32_t { return c0_ + (uint32_t)lane < n ? ops[c0_ + (uint32_t)lane] : 0u; };
        // Round 5: the ops come in GROUPS of steps (G loads out at once), and the group behind the one being walked is asked for when its
        // predecessor is entered: a hit was a chain of some 25 dependent steps of 3.8 us each (one 256-byte load a step, one step
        // ahead); it is a chain of groups now.  win_take(G, c0): the 64 ops of the step at c0 (a multiple of 64 from the pass's start;
        // behind a jump the window is refilled).
#define RB_GW_GROUP 1  // passes 1 and 2: with a checkpoint in front of every step they are walks of one or two steps, and every step asked for
                       // beyond them is a load for nothing (groups of 2 / 3 / 4 in all passes: 7.68 / 8.49 / 8.85 ms on the irregular workload)
#define RB_GW_GROUP3 2 // pass 3 walks ia .. ib, known in advance (eight steps on the bench's windows; past ib no load is issued) -- and still
                       // does not gain from loads further ahead: groups of 2 / 4 / 8 with passes 1 and 2 at one: 7.64 / 7.82 / 8.28 ms.  What a
                       // larger group adds is the selects of win_take and the copies between the two groups; the kernel is bound by what it
                       // issues (its steps are full of wave-uniform decisions: 286 scalar instructions beside 387 vector ones in the
                       // general step of pass 3), not by its loads -- two, three or four waves per SIMD take the same time
        constexpr int RB_GW_GMAX = RB_GW_GROUP > RB_GW_GROUP3 ? RB_GW_GROUP : RB_GW_GROUP3;
        using rb_g12 = std::integral_constant<int, RB_GW_GROUP>;
        using rb_g3 = std::integral_constant<int, RB_GW_GROUP3>;
        uint32_t wc[RB_GW_GMAX], wx[RB_GW_GMAX];
        uint32_t wcb = 0xFFFFFFFFu, wxb = 0xFFFFFFFFu; // first op of the current group / of the group ahead (none)
        auto win_fill = [&](auto G_, uint32_t base, uint32_t (&dst)[RB_GW_GMAX], auto &&ldf) {
            constexpr int G = decltype(G_)::value;
#pragma unroll
            for (int k = 0; k < G; k++) dst[k] = ldf(base + 64u * (uint32_t)k);
        };
        auto win_take = [&](auto G_, uint32_t c0_, auto &&ldf) -> uint32_t {
            constexpr int G = decltype(G_)::value;
            const uint32_t d = c0_ - wcb;
            if (wcb == 0xFFFFFFFFu || d >= 64u * G || (d & 63u)) { // not in the current group
                if (c0_ == wxb) {
#pragma unroll
                    for (int k = 0; k < G; k++) wc[k] = wx[k];
                } else {
                    win_fill(G_, c0_, wc, ldf);
                }
                wcb = c0_, wxb = c0_ + 64u * G;
                win_fill(G_, wxb, wx, ldf); // (the group behind it: out now, wanted G steps from now)
            }
            const uint32_t k = (c0_ - wcb) >> 6;
            uint32_t v = wc[0];
#pragma unroll
            for (int q = 1; q < G; q++) v = k == (uint32_t)q ? wc[q] : v;
            return v;
        };
        auto win_reset = [&]() { wcb = wxb = 0xFFFFFFFFu; };
        for (uint32_t c0 = c_start; c0 < n; c0 += 64u) {
            const uint32_t i = c0 + (uint32_t)lane;
            const uint32_t wv = win_take(rb_g12{}, c0, ld);
            uint32_t opc = rb_opc(wv), len = i < n ? rb_len(wv) : 0u;
            if (opc == RB_OP_CONT) opc = rb_wopc(ops, i), len = rb_wlen(ops, i); // (walk form: one more op of its owner's type)
            const bool isref = opc <= 8u && rb_in(RB_REF_MASK, opc);
            const uint32_t iu = rb_wave_scan_incl(len), ir = rb_wave_scan_incl(isref ? len : 0u);
            if (!first_seen) {
                const uint64_t m = __ballot(len != 0u);
                if (m) {
                    first_seen = true;
                    wrapped = t_st == 0 && !((__ballot(isref) >> __builtin_ctzll(m)) & 1ull);
                }
            }
            if (len) {
                const uint64_t U = Ub + iu - len;
                const int64_t tpos = (int64_t)t_st - 1 + (int64_t)(Rb + ir - (isref ? len : 0u));
                if (isref) { // units U .. U + len - 1 hold tpos + 1 .. tpos + len
                    if (ps > tpos && ps <= tpos + (int64_t)len) {
                        const uint64_t u = U + (uint64_t)(ps - tpos - 1);
                        s_lo = s_lo < u ? s_lo : u, s_hi = s_hi > u ? s_hi : u;
                    }
                    if (pe > tpos && pe <= tpos + (int64_t)len) {
                        const uint64_t u = U + (uint64_t)(pe - tpos - 1);
                        e_lo = e_lo < u ? e_lo : u, e_hi = e_hi > u ? e_hi : u;
                    }
                } else {
                    if (ps == tpos && tpos >= 0) s_lo = s_lo < U ? s_lo : U, s_hi = s_hi > U + len - 1 ? s_hi : U + len - 1;
                    if (pe == tpos && tpos >= 0) e_lo = e_lo < U ? e_lo : U, e_hi = e_hi > U + len - 1 ? e_hi : U + len - 1;
                }
            }
            Ub += rb_readlane<uint32_t>(iu, 63);
            Rb += rb_readlane<uint32_t>(ir, 63);
            if ((int64_t)t_st - 1 + (int64_t)Rb > pe) break; // every unit behind this step lies behind the window's last base
            // every unit at position ps is behind us: on to the checkpoint in front of the units at pe (a long window is not walked)
            if (c_end1 > c0 + 64u && (int64_t)t_st - 1 + (int64_t)Rb > ps) {
                c0 = c_end1 - 64u;
                Ub = cp_e1.x, Rb = cp_e1.y;
                c_end1 = 0;
            }
        }
        if (wrapped) { // an unsorted tpos_aln: binary_search returns what its probe sequence leads to (serial replay)
            if (lane == 0) rb_generic_serial_hit(p, g);
            continue;
        }
        const uint64_t N = rec_units; // all units of the (normalised) record
        s_lo = rb_wave_min_u64(s_lo), s_hi = rb_wave_max_u64(s_hi), e_lo = rb_wave_min_u64(e_lo), e_hi = rb_wave_max_u64(e_hi);
        if (s_lo == ~0ull || e_lo == ~0ull) { // binary_search Err -> panic (liftover.rs:31, :42)
            w.status = RB_ST_PANIC_NOTFOUND;
            if (lane == 0) *row = w;
            continue;
        }
        const uint64_t ks = p.policy == RB_BSEARCH_LEGACY ? rb_legacy_probe(N, s_lo, s_hi) : s_hi;
        const uint64_t ke = p.policy == RB_BSEARCH_LEGACY ? rb_legacy_probe(N, e_lo, e_hi) : e_hi;
        // ---- pass 2: a = first match-type unit >= ks (else N); b = last match-type unit <= ke (else 0) ----
        uint64_t a = N, b = 0, Ra = 0, Qa = 0, Ma = 0, nRb = 0, nQb = 0, nMb = 0, Ua_op = 0, Ub_op = 0;
        uint32_t ia = 0, ib = 0, len_a = 0, len_b = 0;
        bool a_set = false, b_set = false;
        {
            uint64_t U0 = cp0.x, R0 = cp0.y, Q0 = cp0.z, M0 = cp0.w; // (ks, the unit the start resolves to, lies behind the checkpoint too)
            // b is looked for from the checkpoint in front of unit ke; if the stretch from there to ke holds no match-type unit, the
            // walk is done again without the jump (jump2 = 0)
            uint32_t c_end2 = 0;
            uint4 cp_e2 = cp0;
            if (gcp && ke >= ks) {
                const uint32_t k3 = cp_search(0, ke);
                if (k3 * RB_GCP > c_start + RB_GCP) c_end2 = k3 * RB_GCP, cp_e2 = gcp[k3];
            }
          for (int attempt = 0; attempt < 2; attempt++) {
            bool jumped = false;
            if (attempt) U0 = cp0.x, R0 = cp0.y, Q0 = cp0.z, M0 = cp0.w, a_set = false, b_set = false, a = N, b = 0, c_end2 = 0;
            win_reset();
            for (uint32_t c0 = c_start; c0 < n; c0 += 64u) {
                if (a_set && U0 > ke) break; // (nothing behind this can be <= ke)
                const uint32_t i = c0 + (uint32_t)lane;
                const uint32_t wv = win_take(rb_g12{}, c0, ld);
                uint32_t opc = rb_opc(wv), len = i < n ? rb_len(wv) : 0u;
                if (opc == RB_OP_CONT) opc = rb_wopc(ops, i), len = rb_wlen(ops, i);
                const bool okc = opc <= 8u;
                const bool isref = okc && rb_in(RB_REF_MASK, opc), isq = okc && rb_in(RB_QRY_MASK, opc), ism = okc && rb_in(RB_MATCH_MASK, opc);
                const uint32_t iu = rb_wave_scan_incl(len), ir = rb_wave_scan_incl(isref ? len : 0u), iq = rb_wave_scan_incl(isq ? len : 0u),
                               im = rb_wave_scan_incl(ism ? len : 0u);
                const uint64_t U = U0 + iu - len, R = R0 + ir - (isref ? len : 0u), Q = Q0 + iq - (isq ? len : 0u), M = M0 + im - (ism ? len : 0u);
                if (!a_set) {
                    const uint64_t m = __ballot(ism && len != 0u && U + len > ks);
                    if (m) {
                        const int l = __builtin_ctzll(m);
                        const uint64_t Ul = rb_readlane<uint64_t>(U, l);
                        a = ks > Ul ? ks : Ul;
                        const uint64_t off = a - Ul;
                        Ra = rb_readlane<uint64_t>(R, l) + off, Qa = rb_readlane<uint64_t>(Q, l) + off, Ma = rb_readlane<uint64_t>(M, l) + off;
                        Ua_op = Ul, ia = c0 + (uint32_t)l, len_a = rb_readlane<uint32_t>(len, l);
                        a_set = true;
                    }
                }
                {
                    const uint64_t m = __ballot(ism && len != 0u && U <= ke);
                    if (m) {
                        const int l = 63 - __builtin_clzll(m);
                        const uint64_t Ul = rb_readlane<uint64_t>(U, l);
                        const uint32_t ll = rb_readlane<uint32_t>(len, l);
                        b = Ul + ll - 1 < ke ? Ul + ll - 1 : ke;
                        const uint64_t off = b - Ul;
                        nRb = rb_readlane<uint64_t>(R, l) + off + 1, nQb = rb_readlane<uint64_t>(Q, l) + off + 1, nMb = rb_readlane<uint64_t>(M, l) + off + 1;
                        Ub_op = Ul, ib = c0 + (uint32_t)l, len_b = ll;
                        b_set = true;
                    }
                }
                U0 += rb_readlane<uint32_t>(iu, 63), R0 += rb_readlane<uint32_t>(ir, 63), Q0 += rb_readlane<uint32_t>(iq, 63), M0 += rb_readlane<uint32_t>(im, 63);
                if (a_set && c_end2 > c0 + 64u) { // a is known: straight to the checkpoint in front of unit ke
                    c0 = c_end2 - 64u;
                    U0 = cp_e2.x, R0 = cp_e2.y, Q0 = cp_e2.z, M0 = cp_e2.w;
                    c_end2 = 0, jumped = true, b_set = false;
                }
            }
            if (!jumped || b_set) break; // (jumped and found nothing behind the jump: the last match-type unit <= ke lies in what was skipped)
          }
        }
        if (a > b || a >= N || !a_set || !b_set) { // liftover.rs:52-54
            w.status = RB_ST_NONE_INDEL;
            if (lane == 0) *row = w;
            continue;
        }
        w.t_st = t_st + Ra; // liftover.rs:57-60, :77-82 (a and b are match-type units)
        w.t_en = t_st + nRb;
        if (!minus) w.q_st = q_st + Qa, w.q_en = q_st + nQb;
        else w.q_st = q_en - nQb, w.q_en = q_en - Qa;
        w.nmatch = (uint32_t)(nMb - Ma);
        w.aln_len = (uint32_t)(b - a + 1);
        // ---- pass 3: ops ia .. ib, zero lengths dropped, first / last cut, runs of one type merged ----
        uint64_t off;
        if (!reserve((ib - ia + 2u + 3u) & ~3u, &off)) { // (at least as many slots as the merge leaves; + 1: a clip that begins in the bases of a continuation word)
            if (lane == 0) *row = w;
            continue;
        }
        uint32_t out_pos = 0, c_tot = 0, c_opc = 0;
        bool has_carry = false;
        auto ld3 = [&](uint32_t c0_) -> uint32_t {
            const uint32_t i_ = c0_ + (uint32_t)lane;
            return (i_ >= ia && i_ <= ib) ? ops[i_] : 0u;
        };
        win_reset();
        for (uint32_t c0 = ia & ~63u; c0 <= ib; c0 += 64u) {
            const uint32_t i = c0 + (uint32_t)lane;
            const uint32_t wv = win_take(rb_g3{}, c0, ld3);
            uint32_t opc = rb_opc(wv), len = rb_len(wv);
            if (opc == RB_OP_CONT) opc = rb_wopc(ops, i), len = rb_wlen(ops, i);
            const bool in = i >= ia && i <= ib && len != 0u;
            uint32_t piece = len;
            if (i == ia) piece = ia == ib ? (uint32_t)(b - a + 1) : (uint32_t)(Ua_op + len_a - a);
            else if (i == ib) piece = (uint32_t)(b - Ub_op + 1);
            // Round 5: the step that needs none of the machinery below -- every op of the range kept (no zero length), a plain word, no two
            // neighbours of one type (the run carried over is lane 0's neighbour): the ops leave as they are, cut at the ends, and the
            // last one is carried.  An irregular record is irregular in a few places; this is the step of all its other ops (the
            // general step is some 390 vector instructions for 64 ops, and the kernel is bound by them).
            {
                const bool inr = i >= ia && i <= ib;
                const uint32_t ptype = rb_prev_lane(opc, has_carry ? c_opc : 0xFFu);
                const bool odd = inr && (len == 0u || rb_opc(wv) == RB_OP_CONT || (piece >> RB_LEN_BITS_WORD) != 0u || (ptype == opc && (lane == 0 || i > ia)));
                if (!__ballot(odd)) {
                    if (has_carry) {
                        if (lane == 0) rb_emit_run(p.out_ops + off + out_pos, c_tot, c_opc);
                        out_pos += 1u + ((c_tot >> RB_LEN_BITS_WORD) ? 1u : 0u);
                    }
                    const uint64_t im = __ballot(inr); // (not empty: the loop runs over the steps of ia .. ib)
                    const uint32_t cnt = (uint32_t)__builtin_popcountll(im), rank = (uint32_t)__builtin_popcountll(im & ((1ull << lane) - 1ull));
                    if (inr && rank + 1u < cnt) p.out_ops[off + out_pos + rank] = (piece << 4) | opc;
                    out_pos += cnt - 1u;
                    const int last = 63 - __builtin_clzll(im);
                    c_tot = rb_readlane<uint32_t>(piece, last), c_opc = rb_readlane<uint32_t>(opc, last);
                    has_carry = true;
                    continue;
                }
            }
            // code of the last kept op in front of this lane (bit 4: there is one); lane 0 takes the run carried over
            const uint32_t key = in ? ((uint32_t)lane << 5) | 16u | opc : 0u;
            const uint32_t incl = rb_wave_scan_incl_max_u32(key);
            const uint32_t ckey = has_carry ? 16u | c_opc : 0u;
            uint32_t prev = rb_prev_lane(incl, ckey);
            prev = (prev & 16u) ? prev : ckey; // (no kept op in front of this lane in this step: the run carried over)
            const bool start = in && !((prev & 16u) && (prev & 15u) == opc);
            const uint64_t sm = __ballot(start);
            const uint32_t nstarts = (uint32_t)__builtin_popcountll(sm);
            const int32_t ridx = (int32_t)__builtin_popcountll(sm & ((2ull << lane) - 1ull)) - 1; // run of this lane inside the step (-1: the carried one)
            run_tot[lane] = 0u;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if (in && ridx >= 0) atomicAdd(&run_tot[ridx], piece);
            if (start) run_opc[ridx] = opc;
            c_tot += rb_wave_sum_u32((in && ridx < 0) ? piece : 0u);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if (nstarts) { // (runs of 2^28 bases and more leave as two words: rb_emit_run)
                if (has_carry) {
                    const uint32_t cw = 1u + ((c_tot >> RB_LEN_BITS_WORD) ? 1u : 0u);
                    if (lane == 0) rb_emit_run(p.out_ops + off + out_pos, c_tot, c_opc);
                    out_pos += cw;
                }
                const bool mine_out = (uint32_t)lane + 1u < nstarts;
                const uint32_t my_tot = mine_out ? run_tot[lane] : 0u;
                const uint32_t my_words = mine_out ? 1u + ((my_tot >> RB_LEN_BITS_WORD) ? 1u : 0u) : 0u;
                const uint32_t wincl = rb_wave_scan_incl(my_words);
                if (mine_out) rb_emit_run(p.out_ops + off + out_pos + (wincl - my_words), my_tot, run_opc[lane]);
                out_pos += rb_readlane<uint32_t>(wincl, 63);
                c_tot = run_tot[nstarts - 1u], c_opc = run_opc[nstarts - 1u];
                has_carry = true;
            }
            __builtin_amdgcn_wave_barrier();
        }
        if (has_carry) {
            if (lane == 0) rb_emit_run(p.out_ops + off + out_pos, c_tot, c_opc);
            out_pos += 1u + ((c_tot >> RB_LEN_BITS_WORD) ? 1u : 0u);
        }
        w.out_n = out_pos;
        w.out_off = off;
        if (lane == 0) *row = w;
    }
}

// out_ops_used / out_ops_needed from the arena cursors
__global__ __launch_bounds__(64) void rb_k_finish(rb_lift_params p) {
    unsigned long long mx = 0, sum = 0;
    for (uint32_t a = threadIdx.x; a < p.n_arena; a += 64) {
        const unsigned long long c = p.arena_cur[(uint64_t)a * RB_ARENA_STRIDE];
        mx = c > mx ? c : mx;
        sum += c;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(mx, off, 64);
        mx = o > mx ? o : mx;
        sum += __shfl_xor(sum, off, 64);
    }
    if (threadIdx.x != 0) return;
    p.counters->out_ops_used = p.arena_origin + sum;
    // what makes the job fit: the slots the window lists ask for, plus every arena as large as the fullest one got
    p.counters->out_ops_needed = p.needed_base + (mx + 3ull) / 4ull * 4ull * p.n_arena + 1024ull * p.n_arena;
    if (p.counters->n_hits > p.rows_cap) p.counters->overflow = 1;
    if (p.n_tiles && !p.debug_skip) { // (the diagnostics words, outside the diagnostics builds: how the short records went)
        p.counters->phase[3] = p.n_tiles;
        p.counters->phase[4] = (uint32_t)*p.fb_count; // records the tile kernel handed to the per-record kernel
    }
    if (p.brk_mode && p.counters->brk_scratch_short) { // one of the scratch-row cursors ran out before the rows did: ask for a quarter more
        p.counters->overflow = 1;
        const uint64_t have = p.counters->n_hits > p.rows_cap ? p.counters->n_hits : p.rows_cap;
        p.counters->n_hits = have + have / 4u + 1024u;
    }
}

// one-walk break-paf: the rows of a record leave their scratch place for rows_final[hit_off[r] ..] (hit_off scanned by now)
__global__ __launch_bounds__(256) void rb_k_break_gather(rb_lift_params p) {
    // four lanes per record, 16 bytes of a 64-byte row each (a record has a handful of pieces: a wavefront per record idles)
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint64_t r = t >> 2;
    if (r >= p.n_rec) return;
    const uint64_t h0 = p.hit_off[r], n = p.hit_off[r + 1] - h0, src = p.brk_off[r];
    if (src == ~0ull) return;
    const uint32_t part = (uint32_t)(t & 3u);
    const uint4 *from = reinterpret_cast<const uint4 *>(p.rows + src);
    uint4 *to = reinterpret_cast<uint4 *>(p.rows_final + h0);
    for (uint64_t j = 0; j < n; j++)
        if (h0 + j < p.rows_cap) to[4 * j + part] = from[4 * j + part];
}
extern "C" hipError_t rb_launch_break_gather(const rb_lift_params *p, hipStream_t stream) {
    if (p->n_rec == 0) return hipSuccess;
    hipLaunchKernelGGL(rb_k_copy_clips, dim3(2048), dim3(256), 0, stream, *p); // (clips without a slot: their rows are still where the list says)
    hipLaunchKernelGGL(rb_k_break_gather, dim3((unsigned)((p->n_rec * 4 + 255) / 256)), dim3(256), 0, stream, *p);
    return hipGetLastError();
}
// one-walk break-paf: the pieces of the records the clip kernel declined get their rows (in the final array, hit_off scanned by
// now) and their entries in the generic list; then the generic kernel clips them (p.rows = the final rows, p.x_st / x_en = the
// windows rb_k_break_pieces wrote in list mode) and rb_k_finish sums up
__global__ __launch_bounds__(256) void rb_k_break_list_declined(rb_lift_params p) {
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (r >= p.n_rec || p.brk_off[r] != ~1ull) return;
    p.brk_off[r] = ~0ull; // (the gather leaves the record alone)
    p.hit_off[r] = 0;     // (rb_k_break_pieces counts its pieces next)
    p.brk_decl_list[atomicAdd(p.brk_decl_count, 1ull)] = (uint32_t)r;
}
extern "C" hipError_t rb_launch_break_list_declined(const rb_lift_params *p, hipStream_t stream) {
    if (p->n_rec == 0) return hipSuccess;
    hipLaunchKernelGGL(rb_k_break_list_declined, dim3((unsigned)((p->n_rec + 255) / 256)), dim3(256), 0, stream, *p);
    return hipGetLastError();
}
__global__ __launch_bounds__(256) void rb_k_break_declined_rows(rb_lift_params p) {
    const uint64_t n_list = *p.brk_decl_count;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n_list; i += (uint64_t)gridDim.x * 256u) {
        const uint32_t r = p.brk_decl_list[i];
        const uint64_t h0 = p.hit_off[r], n = p.hit_off[r + 1] - h0;
        for (uint64_t j = 0; j < n; j++) {
            const uint64_t h = h0 + j;
            if (h >= p.rows_cap) break;
            rb_hit_row *row = &p.rows[h];
            row->rec = r;
            row->win = (uint32_t)j;
            row->flags = RB_HIT_GENERIC;
            const unsigned long long g = atomicAdd((unsigned long long *)&p.counters->n_generic, 1ull);
            p.gen_list[g] = (uint32_t)h;
        }
    }
}
extern "C" hipError_t rb_launch_break_declined(const rb_lift_params *p, hipStream_t stream) {
    if (p->n_rec == 0) return hipSuccess;
    hipLaunchKernelGGL(rb_k_break_declined_rows, dim3((unsigned)std::min<uint64_t>((p->n_rec + 255) / 256, 256)), dim3(256), 0, stream, *p);
    if (p->gen_cp) hipLaunchKernelGGL(rb_k_generic_checkpoints, dim3(2048), dim3(256), 0, stream, *p);
    hipLaunchKernelGGL(rb_k_generic_jobs, dim3(1024), dim3(256), 0, stream, *p);
    hipLaunchKernelGGL(rb_k_liftover_generic_wave, dim3(2048), dim3(256), 0, stream, *p);
    hipLaunchKernelGGL(rb_k_finish, dim3(1), dim3(64), 0, stream, *p);
    return hipGetLastError();
}
extern "C" hipError_t rb_launch_count_and_scan(const rb_lift_params *p, uint64_t *block_sums, bool do_count, hipStream_t stream) {
    if (p->n_rec == 0) return hipSuccess;
    if (do_count) {
        const unsigned blocks = (unsigned)((p->n_rec + 255) / 256);
        hipLaunchKernelGGL(rb_k_count_hits, dim3(blocks), dim3(256), 0, stream, *p);
    }
    return rb_launch_exclusive_scan(p->hit_off, p->n_rec, block_sums, &p->counters->n_hits, stream);
}
// in-place exclusive scan of n u64 counts (n + 1 outputs); block_sums: rb_scan_block_sums_count(n) words of scratch
extern "C" hipError_t rb_launch_exclusive_scan(uint64_t *v, uint64_t n, uint64_t *block_sums, uint64_t *total_out, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const uint64_t nb = (n + RB_SCAN_PER_BLOCK - 1) / RB_SCAN_PER_BLOCK;
    hipLaunchKernelGGL(rb_k_scan_partial, dim3((unsigned)nb), dim3(256), 0, stream, (const uint64_t *)v, n, block_sums);
    hipLaunchKernelGGL(rb_k_scan_top, dim3(1), dim3(256), 0, stream, block_sums, nb);
    hipLaunchKernelGGL(rb_k_scan_apply, dim3((unsigned)nb), dim3(256), 0, stream, v, n, (const uint64_t *)block_sums, total_out);
    return hipGetLastError();
}
extern "C" hipError_t rb_launch_make_jobs(const rb_lift_params *p, hipStream_t stream) {
    if (p->n_rec == 0) return hipSuccess;
    hipLaunchKernelGGL(rb_k_make_jobs, dim3((unsigned)((p->n_rec + 255) / 256)), dim3(256), 0, stream, *p);
    return hipGetLastError();
}

extern "C" hipError_t rb_launch_liftover_stream(const rb_lift_params *p, hipStream_t stream) {
    if (p->n_rec == 0 || p->wave_end <= p->wave0) return hipSuccess;
    const unsigned blocks = (unsigned)(((uint64_t)(p->wave_end - p->wave0) + 3) / 4);
    if (p->debug_skip) { // diagnostics only (bench.py --debug-skip, the box block's clock stamps)
        if (!p->brk_mode) {
            hipLaunchKernelGGL(rb_k_liftover_stream_diag, dim3(blocks), dim3(256), 0, stream, *p);
            return hipGetLastError();
        }
    }
    if (p->brk_mode) return rb_launch_liftover_stream_brk(p, blocks, stream);
    hipLaunchKernelGGL(rb_k_liftover_stream, dim3(blocks), dim3(256), 0, stream, *p);
    return hipGetLastError();
}
extern "C" hipError_t rb_launch_liftover_tail(const rb_lift_params *p, hipStream_t stream) {
    if (p->n_rec == 0) return hipSuccess;
    hipLaunchKernelGGL(rb_k_copy_clips, dim3(2048), dim3(256), 0, stream, *p);
    if (p->gen_cp) hipLaunchKernelGGL(rb_k_generic_checkpoints, dim3(2048), dim3(256), 0, stream, *p);
    hipLaunchKernelGGL(rb_k_generic_jobs, dim3(1024), dim3(256), 0, stream, *p);
    hipLaunchKernelGGL(rb_k_liftover_generic_wave, dim3(2048), dim3(256), 0, stream, *p);
    hipLaunchKernelGGL(rb_k_finish, dim3(1), dim3(64), 0, stream, *p);
    return hipGetLastError();
}

extern "C" size_t rb_scan_block_sums_count(uint64_t n_rec) { return (size_t)((n_rec + RB_SCAN_PER_BLOCK - 1) / RB_SCAN_PER_BLOCK + 2); }
