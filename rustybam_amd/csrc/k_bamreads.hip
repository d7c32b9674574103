// k_bamreads.hip -- the per-read index `rb nucfreq` needs of a BAM stream, from the columns of rb_dev_bam_records (gfx950, wave64):
// rb_dev_bam_reads.
//
// Restates what bam_read_records (host/rb_host.cpp) keeps per record besides the columns: where the record's SEQ lies, nf_key(tid, pos),
// the running maximum of nf_key(tid, bam_endpos) over the reads the pileup admits, and the sortedness loop at the top of nucfreq_bam.
//
// Shape.
//   rb_k_bam_reads       a record is a ROW of 16 lanes, four records to a wavefront (the shape of rb_k_bam_copy).  The row sums the
//                        lengths of the record's reference-consuming ops from whole aligned 16-byte groups of ops, RB_BAMREADS_ROW_STEP
//                        = 64 ops per step; a CIGAR of more than RB_BAMREADS_ROW_MAX ops is summed afterwards by the whole wavefront
//                        (256 ops per step).  A lane's 64-bit sum leaves as three 24-bit pieces through the DPP sums of rb_device.h.
//                        Lane 0 of the row writes seq_off, start_key and the read's OWN end key (0: it does not enter the pileup; every
//                        real key is larger).  A wavefront that holds a record out of order sends one 64-bit atomic minimum.
//   the inclusive prefix maximum of the end keys, device-wide: the maxima of workgroups of RB_BAMREADS_SCAN_BLOCK records, those scanned
//   in place (up to RB_BAMREADS_SCAN_BLOCK of them by one workgroup; more: the same two kernels one level up, and a serial top), and an
//   apply pass.  A maximum is order-free, so two calls write the same bytes.
//
// Algorithmic bytes per record: 8 (op_off) + 17 (tid, pos, flag, status) + 8 (rec_off) + 8 of the fixed fields + 4 per op in;
// 24 out; the scan reads the end keys twice and writes them once (24).
#include "rb_device.h"
#include "rb_launch.h"

#define RB_BAMREADS_ROW_STEP 64u   // ops per step of a row of 16 lanes (one 16-byte group per lane)
#define RB_BAMREADS_WAVE_STEP 256u // ... of the whole wavefront
#ifndef RB_BAMREADS_ROW_MAX
#define RB_BAMREADS_ROW_MAX 4096u  // CIGARs of more ops than this are summed by the wavefront (rb_k_bam_copy's line)
#endif
#define RB_BAMREADS_BATCH 4        // steps whose loads are in flight together
#define RB_BAMREADS_SCAN_BLOCK 512u // records (or maxima) per workgroup of the scan: two per thread

extern "C" uint32_t rb_bam_reads_row_step(void) { return RB_BAMREADS_ROW_STEP; }
extern "C" uint32_t rb_bam_reads_row_max(void) { return RB_BAMREADS_ROW_MAX; }
extern "C" uint32_t rb_bam_reads_wave_step(void) { return RB_BAMREADS_WAVE_STEP; }
extern "C" uint32_t rb_bam_reads_scan_block(void) { return RB_BAMREADS_SCAN_BLOCK; }
// maxima of every level of the scan over n records
extern "C" size_t rb_bam_reads_blk_count(uint64_t n) {
    const uint64_t nb0 = (n + RB_BAMREADS_SCAN_BLOCK - 1) / RB_BAMREADS_SCAN_BLOCK;
    const uint64_t nb1 = (nb0 + RB_BAMREADS_SCAN_BLOCK - 1) / RB_BAMREADS_SCAN_BLOCK;
    return (size_t)(nb0 + nb1 + 2);
}

__device__ __forceinline__ uint64_t rb_nf_key(const int32_t tid, const uint64_t p) {
    return ((uint64_t)(uint32_t)tid << 32) | (p < 0xFFFFFFFFull ? p : 0xFFFFFFFFull);
}

// The reference span of ops[a .. e) by W lanes (16: a row, every row of the wavefront its own CIGAR; 64: the wavefront): every lane of
// the W gets the sum.  Only aligned groups that hold a word of the CIGAR are loaded.
template <int W>
__device__ __forceinline__ uint64_t rb_bam_reads_ref(const uint32_t *ops, const uint64_t a, const uint64_t e, const bool take, const uint32_t gl) {
    static_assert((W == 16 && 4 * W == RB_BAMREADS_ROW_STEP) || (W == 64 && 4 * W == RB_BAMREADS_WAVE_STEP), "a step is one 16-byte group per lane");
    uint64_t s = 0;
    if (take) {
        for (uint64_t g0 = (a & ~3ull) + 4u * gl; g0 < e; g0 += (uint64_t)RB_BAMREADS_BATCH * (4u * W)) {
            uint4 pf[RB_BAMREADS_BATCH];
#pragma unroll
            for (int b = 0; b < RB_BAMREADS_BATCH; b++) {
                const uint64_t g = g0 + (uint64_t)b * (4u * W);
                pf[b] = g < e ? *reinterpret_cast<const uint4 *>(ops + g) : make_uint4(0u, 0u, 0u, 0u);
            }
#pragma unroll
            for (int b = 0; b < RB_BAMREADS_BATCH; b++) {
                const uint64_t g = g0 + (uint64_t)b * (4u * W);
                const uint32_t w[4] = {pf[b].x, pf[b].y, pf[b].z, pf[b].w};
#pragma unroll
                for (int q = 0; q < 4; q++)
                    if (g + (uint32_t)q >= a && g + (uint32_t)q < e && rb_in(RB_REF_MASK, rb_opc(w[q]))) s += rb_len(w[q]);
            }
        }
    }
    // (s < 2^60: fewer than 2^32 ops of less than 2^28) three pieces of 24 bits, so that the sum of 64 of them fits a dword
    uint32_t p0 = (uint32_t)s & 0xFFFFFFu, p1 = (uint32_t)(s >> 24) & 0xFFFFFFu, p2 = (uint32_t)(s >> 48);
    if (W == 16) p0 = rb_row_sum(p0), p1 = rb_row_sum(p1), p2 = rb_row_sum(p2);
    else p0 = rb_wave_sum_u32(p0), p1 = rb_wave_sum_u32(p1), p2 = rb_wave_sum_u32(p2);
    return (uint64_t)p0 + ((uint64_t)p1 << 24) + ((uint64_t)p2 << 48);
}

__global__ __launch_bounds__(256) void rb_k_bam_reads(rb_bam_reads_params p) {
    const int lane = rb_lane();
    const uint32_t gl = (uint32_t)lane & 15u;
    const uint64_t k0 = ((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6)) * 4u; // the wavefront's first record
    const uint64_t k = k0 + ((uint32_t)lane >> 4);
    const bool live = k < p.n;
    uint64_t a = 0, e = 0;
    if (live) a = p.op_off[k], e = p.op_off[k + 1];
    const bool is_long = live && e - a > (uint64_t)RB_BAMREADS_ROW_MAX;
    uint64_t ref = rb_bam_reads_ref<16>(p.ops, a, e, live && !is_long, gl);
    // ---- the long CIGARs of these four records, one after the other, by the whole wavefront ----
    unsigned long long todo = rb_ballot(is_long && gl == 0u);
    while (todo) {
        const int b = __builtin_ctzll(todo);
        todo &= todo - 1ull;
        const uint64_t s = rb_bam_reads_ref<64>(p.ops, rb_readlane<uint64_t>(a, b), rb_readlane<uint64_t>(e, b), true, (uint32_t)lane);
        if (((uint32_t)lane >> 4) == ((uint32_t)b >> 4)) ref = s;
    }
    const bool mine = live && gl == 0u;
    bool cand = false;
    if (mine) {
        const int32_t tid = p.tid[k];
        const int64_t pos = p.pos[k];
        const uint32_t flag = p.flag[k];
        const bool ok = p.status[k] == RB_BAM_OK;
        uint64_t so = 0;
        if (ok) { // (a refused record may be shorter than its fixed fields)
            const uint64_t R = p.rec_off[k];
            const uint64_t h = rb_bam_bytes(p.data, R + 8u, 8u); // l_read_name, mapq, bin, n_cigar_op, flag
            so = R + 32u + ((uint32_t)h & 0xFFu) + 4ull * ((uint32_t)(h >> 32) & 0xFFFFu);
        }
        const uint64_t sk = rb_nf_key(tid, (uint64_t)pos);
        const bool enters = ok && tid >= 0 && !(flag & (0x4u | 0x100u | 0x200u | 0x400u));
        const uint64_t endpos = (uint64_t)(pos > 0 ? pos : 0) + (((flag & 4u) || ref == 0) ? 1ull : ref); // bam_endpos
        p.seq_off[k] = so;
        p.start_key[k] = sk;
        p.end_key_pmax[k] = enters ? rb_nf_key(tid, endpos) : 0ull;
        if (k >= 1 && tid >= 0 && pos >= 0) cand = sk < rb_nf_key(p.tid[k - 1], (uint64_t)p.pos[k - 1]);
    }
    const unsigned long long out_of_order = rb_ballot(cand);
    if (out_of_order != 0ull && lane == 0) atomicMin(p.first_unsorted, (unsigned long long)(k0 + ((uint32_t)__builtin_ctzll(out_of_order) >> 4)));
}

// ---- the inclusive prefix maximum ----------------------------------------------------------------------
__device__ __forceinline__ uint64_t rb_max64(const uint64_t x, const uint64_t y) { return x > y ? x : y; }

// out[b] = the maximum of workgroup b's RB_BAMREADS_SCAN_BLOCK values
__global__ __launch_bounds__(256) void rb_k_bam_reads_max_partial(const uint64_t *v, const uint64_t n, uint64_t *out) {
    __shared__ uint64_t sh[4];
    const uint64_t i0 = (uint64_t)blockIdx.x * RB_BAMREADS_SCAN_BLOCK + 2u * threadIdx.x;
    uint64_t m = 0;
    if (i0 < n) m = v[i0];
    if (i0 + 1 < n) m = rb_max64(m, v[i0 + 1]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = rb_max64(m, __shfl_xor(m, off, 64));
    if ((threadIdx.x & 63u) == 0u) sh[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = rb_max64(rb_max64(sh[0], sh[1]), rb_max64(sh[2], sh[3]));
}
// the inclusive prefix maximum of one value per thread of the workgroup, on top of `carry`
__device__ __forceinline__ uint64_t rb_block_scan_max(uint64_t m, const uint64_t carry, uint64_t *sh /* [4] */) {
    const int lane = rb_lane();
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint64_t y = __shfl_up(m, off, 64);
        if (lane >= off) m = rb_max64(m, y);
    }
    const uint32_t w = threadIdx.x >> 6;
    __syncthreads(); // (sh may still be read from the call before)
    if (lane == 63) sh[w] = m;
    __syncthreads();
    uint64_t c = carry;
    for (uint32_t j = 0; j < w; j++) c = rb_max64(c, sh[j]);
    return rb_max64(m, c);
}
// one workgroup: the inclusive prefix maximum of blk[0 .. nb), in place
__global__ __launch_bounds__(256) void rb_k_bam_reads_max_top(uint64_t *blk, const uint64_t nb) {
    __shared__ uint64_t sh[4];
    __shared__ uint64_t last;
    uint64_t carry = 0;
    for (uint64_t b = 0; b < nb; b += 256u) {
        const uint64_t i = b + threadIdx.x;
        const uint64_t m = rb_block_scan_max(i < nb ? blk[i] : 0ull, carry, sh);
        if (i < nb) blk[i] = m;
        if (threadIdx.x == 255u) last = m;
        __syncthreads();
        carry = last;
    }
}
// v[i] = max(v[0 .. i]) given blk = the inclusive prefix maxima of the workgroups' maxima
__global__ __launch_bounds__(256) void rb_k_bam_reads_max_apply(uint64_t *v, const uint64_t n, const uint64_t *blk) {
    __shared__ uint64_t sh[4];
    const uint64_t i0 = (uint64_t)blockIdx.x * RB_BAMREADS_SCAN_BLOCK + 2u * threadIdx.x;
    const uint64_t x0 = i0 < n ? v[i0] : 0ull, x1 = i0 + 1 < n ? v[i0 + 1] : 0ull;
    const uint64_t carry = blockIdx.x ? blk[blockIdx.x - 1] : 0ull;
    const uint64_t incl = rb_block_scan_max(rb_max64(x0, x1), carry, sh); // max of everything up to and including x1
    // what lies in front of x0: the thread before, or the carry
    uint64_t before = __shfl_up(incl, 1, 64);
    __shared__ uint64_t wlast[4];
    if ((threadIdx.x & 63u) == 63u) wlast[threadIdx.x >> 6] = incl;
    __syncthreads();
    if ((threadIdx.x & 63u) == 0u) before = threadIdx.x ? wlast[(threadIdx.x >> 6) - 1] : carry;
    if (i0 < n) v[i0] = rb_max64(before, x0);
    if (i0 + 1 < n) v[i0 + 1] = incl;
}

extern "C" hipError_t rb_launch_bam_reads(const rb_bam_reads_params *p, hipStream_t stream) {
    if (p->n == 0) return hipSuccess;
    hipLaunchKernelGGL(rb_k_bam_reads, dim3((unsigned)((p->n + 15) / 16)), dim3(256), 0, stream, *p);
    const uint64_t B = RB_BAMREADS_SCAN_BLOCK;
    const uint64_t nb0 = (p->n + B - 1) / B;
    uint64_t *v = p->end_key_pmax, *b0 = p->blk;
    if (nb0 > 1) {
        hipLaunchKernelGGL(rb_k_bam_reads_max_partial, dim3((unsigned)nb0), dim3(256), 0, stream, (const uint64_t *)v, p->n, b0);
        if (nb0 > B) { // more maxima than one workgroup scans: the same one level up, and the serial top over those
            const uint64_t nb1 = (nb0 + B - 1) / B;
            uint64_t *b1 = b0 + nb0;
            hipLaunchKernelGGL(rb_k_bam_reads_max_partial, dim3((unsigned)nb1), dim3(256), 0, stream, (const uint64_t *)b0, nb0, b1);
            hipLaunchKernelGGL(rb_k_bam_reads_max_top, dim3(1), dim3(256), 0, stream, b1, nb1);
            hipLaunchKernelGGL(rb_k_bam_reads_max_apply, dim3((unsigned)nb1), dim3(256), 0, stream, b0, nb0, (const uint64_t *)b1);
        } else {
            hipLaunchKernelGGL(rb_k_bam_reads_max_top, dim3(1), dim3(256), 0, stream, b0, nb0);
        }
    }
    hipLaunchKernelGGL(rb_k_bam_reads_max_apply, dim3((unsigned)nb0), dim3(256), 0, stream, v, p->n, (const uint64_t *)b0);
    return hipGetLastError();
}
