// k_largest.hip -- liftover --largest (main.rs:200-208) on the device, for gfx950: hit rows reduced to one row per KEY.  The reference sorts
// the records trim_paf_by_rgns returned stably by id and keeps, per id, the LAST record of maximal t_en - t_st.  The host interns the id
// strings into dense keys; hit rows lie in the order of that record list, so "the last maximum behind a stable sort" is "the largest row
// index among the key's rows of the largest span": two atomic maxima, one kernel apart, and a scan over the keys.
//   rb_k_largest_pass<1>  best_span[key] = max span           rb_k_largest_pass<2>  best_row[key] = max (row + 1) among rows of that span
//   rb_k_largest_flag, the library's exclusive scan, rb_k_largest_place           sel[] = the winners, dense, in ascending key order
// Spans are whole u64 and the row index is a u64 of its own: nothing is packed into one word.  The result does not depend on the order
// in which the atomics arrive (a maximum is the same in any order), so two calls on the same rows give the same bytes.
#include "rb_device.h"
#include "rb_launch.h"

// what the atomics have left at `a` so far.  A device-scope load: it is served behind the vector cache, where a line fetched early would
// go on saying 0 for as long as it stays.  An old value is only ever too SMALL (the maxima grow), so skipping the atomic when the stored
// value is already as large is safe however stale the value is.
__device__ __forceinline__ unsigned long long rb_largest_seen(const unsigned long long *a) {
    return __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One lane per row, two 16-byte loads of its 64 bytes: {rec, win, status | flags << 16, out_n} and {t_st, t_en}.
template <int PASS>
__global__ __launch_bounds__(256) void rb_k_largest_pass(rb_largest_params p) {
    const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const int lane = rb_lane();
    uint4 a = make_uint4(0, 0, RB_ST_NONE_EMPTY, 0), b = make_uint4(0, 0, 0, 0); // (a lane behind the last row: a row that does not take part)
    if (k < p.n_rows) {
        const uint4 *r = reinterpret_cast<const uint4 *>(p.rows + k);
        a = r[0], b = r[1];
    }
    const uint32_t status = a.z & 0xFFFFu, flags = a.z >> 16;
    const bool ok = status == RB_ST_OK; // (rows of any other status take no part: the reference dropped them or panicked)
    uint32_t key = 0xFFFFFFFFu;
    bool part = false;
    if (ok) {
        if (!(flags & RB_HIT_INSIDE)) key = p.win_key[a.y], part = true; // liftover.rs:20: the window's id
        else if (p.rec_key) key = p.rec_key[a.x], part = true;           // liftover.rs:23-25: the record's own
        part = part && (uint64_t)key < p.n_keys;
    }
    const uint64_t span = (((uint64_t)b.w << 32) | b.z) - (((uint64_t)b.y << 32) | b.x);
    if (PASS == 1) {
        const unsigned long long bad = rb_ballot(ok && !part);
        if (bad && lane == __builtin_ctzll(bad)) atomicAdd(&p.out[1], (unsigned long long)__builtin_popcountll(bad));
        if (p.worst_status) {
            const unsigned long long pan = rb_ballot(status >= RB_ST_PANIC_NOTFOUND);
            if (pan && lane == __builtin_ctzll(pan)) atomicMax(p.worst_status, status);
        }
    }
    // the rows this pass has something to say about: every row that takes part / the rows that hold their key's largest span
    const bool mine = PASS == 1 ? part : part && span == p.best_span[key]; // (pass 2 starts behind the kernel boundary: best_span is final)
    const unsigned long long mm = rb_ballot(mine);
    if (mm == 0) return;
    // All INSIDE rows of unstripped records share the key of the empty id, and windows that repeat an id share theirs: when every such lane
    // of the wave holds ONE key the wave settles it among its lanes and sends one atomic.  The lane that speaks is the last one: in pass 2
    // it holds the largest row index.
    const int last = 63 - __builtin_clzll(mm);
    const uint32_t key_w = rb_readlane<uint32_t>(key, last);
    const bool uniform = rb_ballot(mine && key != key_w) == 0;
    if (PASS == 1) {
        uint64_t m = mine ? span : 0;
        if (uniform) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const uint64_t o = __shfl_xor(m, off, 64);
                m = o > m ? o : m;
            }
        }
        if (mine && (!uniform || lane == last) && rb_largest_seen(&p.best_span[key]) < m) atomicMax(&p.best_span[key], (unsigned long long)m);
    } else {
        // (k + 1: a key whose only row is row 0 -- or whose only span is 0, which pass 1 never had to store -- is still told from a key without rows)
        if (mine && (!uniform || lane == last) && rb_largest_seen(&p.best_row[key]) < k + 1) atomicMax(&p.best_row[key], (unsigned long long)(k + 1));
    }
}

// the compaction over the keys: 1 for a key with a winner, the library's exclusive scan over those (deterministic: block sums, no atomics),
// then every winner to its slot
__global__ __launch_bounds__(256) void rb_k_largest_flag(rb_largest_params p) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < p.n_keys) p.best_span[i] = p.best_row[i] != 0 ? 1ull : 0ull;
}
__global__ __launch_bounds__(256) void rb_k_largest_place(rb_largest_params p) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= p.n_keys) return;
    const unsigned long long r = p.best_row[i];
    if (r != 0) p.sel[p.best_span[i]] = r - 1;
}

extern "C" hipError_t rb_launch_largest(const rb_largest_params *p, uint64_t *block_sums, hipStream_t stream) {
    if (p->n_rows) {
        const unsigned blocks = (unsigned)((p->n_rows + 255) / 256);
        hipLaunchKernelGGL(rb_k_largest_pass<1>, dim3(blocks), dim3(256), 0, stream, *p);
        if (p->n_keys) hipLaunchKernelGGL(rb_k_largest_pass<2>, dim3(blocks), dim3(256), 0, stream, *p);
    }
    if (p->n_rows == 0 || p->n_keys == 0) return hipGetLastError(); // (n_sel = 0: out was zeroed)
    const unsigned kblocks = (unsigned)((p->n_keys + 255) / 256);
    hipLaunchKernelGGL(rb_k_largest_flag, dim3(kblocks), dim3(256), 0, stream, *p);
    const hipError_t e = rb_launch_exclusive_scan((uint64_t *)p->best_span, p->n_keys, block_sums, (uint64_t *)&p->out[0], stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rb_k_largest_place, dim3(kblocks), dim3(256), 0, stream, *p);
    return hipGetLastError();
}

// ---- around it, for rb_host_liftover_largest_text ----
// The id of a record whose end indels were stripped carries a suffix made of its own CIGAR (paf.rs:726-731), which no key stands for:
// such a record gets a key no key space holds, so an INSIDE row of it shows up in the count of rows left out and the caller declines.
__global__ __launch_bounds__(256) void rb_k_largest_rec_keys(const rb_norm_row *norm, uint64_t n_rec, uint32_t inside_key, uint32_t *rec_key) {
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (r < n_rec) rec_key[r] = (norm[r].flags & RB_F_STRIPPED) ? 0xFFFFFFFFu : inside_key;
}
// the selected rows and the four words at their out_off (the clip descriptor of a row that has one), dense, in the order of sel[]
__global__ __launch_bounds__(256) void rb_k_largest_gather(const rb_hit_row *rows, const uint32_t *out_ops, const uint64_t *sel, uint64_t n_sel,
                                                           rb_hit_row *sel_rows, uint32_t *sel_desc) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n_sel) return;
    const rb_hit_row h = rows[sel[i]];
    sel_rows[i] = h;
    const bool d = h.status == RB_ST_OK && (h.flags & RB_HIT_DESCRIPTOR);
#pragma unroll
    for (int j = 0; j < 4; j++) sel_desc[4 * i + j] = d ? out_ops[h.out_off + j] : 0u;
}
extern "C" hipError_t rb_launch_largest_rec_keys(const rb_norm_row *norm, uint64_t n_rec, uint32_t inside_key, uint32_t *rec_key, hipStream_t stream) {
    if (n_rec == 0) return hipSuccess;
    hipLaunchKernelGGL(rb_k_largest_rec_keys, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, stream, norm, n_rec, inside_key, rec_key);
    return hipGetLastError();
}
extern "C" hipError_t rb_launch_largest_gather(const rb_hit_row *rows, const uint32_t *out_ops, const uint64_t *sel, uint64_t n_sel, rb_hit_row *sel_rows,
                                               uint32_t *sel_desc, hipStream_t stream) {
    if (n_sel == 0) return hipSuccess;
    hipLaunchKernelGGL(rb_k_largest_gather, dim3((unsigned)((n_sel + 255) / 256)), dim3(256), 0, stream, rows, out_ops, sel, n_sel, sel_rows, sel_desc);
    return hipGetLastError();
}
