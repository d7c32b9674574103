// k_nftext.hip -- the lines of `rb nucfreq` printed on the device, gfx950 (wave64, CDNA4).
//
//   rb_k_nft  replaces `impl Display for Nucfreq` (nucfreq.rs:17-33) and the --small lines (nucfreq.rs:148-150) as main.rs prints
//             them, one line per covered position, straight from the counts rb_dev_nucfreq left in HBM.
//
// The unit of work is a RUN: RB_NFT_RUN consecutive positions of one segment, one wavefront, RB_NFT_STEP positions (one per lane) a
// step.  A segment of n positions is ceil(n / RB_NFT_RUN) runs; the host numbers the runs of all segments through (unit0[s] = the
// first run of segment s) and a wavefront finds its segment by bisection of that table.  Run twice: sizes (bytes per run -> the
// device-wide exclusive scan -> where the run's text goes; lines and first covered position per segment on the way), then fill.
//
// Fill: the lines of a step are placed with a wave scan of their lengths and put together in LDS, at the 16-byte phase they have in
// memory; whole 16-byte groups leave with aligned 16-byte stores, and the bytes behind the last whole group stay in the stage as the
// head of the next step.  Only the first and the last group of a RUN can be shared with a neighbour: those leave byte by byte.
//
// Roofline: HBM (byte work, no MFMA).  Algorithmic bytes: 16 B per position read twice + the text written.
#include "rb_device.h"
#include "rb_launch.h"

#define RB_NFT_STEP 64u
#define RB_NFT_RUN 256u                     // positions per wavefront: four steps
#define RB_NFT_BLOCK (4u * RB_NFT_RUN)      // positions per workgroup inside one long segment
#define RB_NFT_FIX 255u                     // longest prefix / suffix
#define RB_NFT_STAGE (4096u + 16u)          // bytes of the stage of one wavefront: up to 15 bytes carried + one round of lines
// a line is at most 255 + 10 + 1 + 10 + 1 + 4 * 10 + 3 + 255 = 575 bytes: one always fits behind 15 carried bytes
static_assert(15u + 2u * RB_NFT_FIX + 65u <= RB_NFT_STAGE, "one line must fit the stage");

extern "C" uint32_t rb_nft_step(void) { return RB_NFT_STEP; }
extern "C" uint32_t rb_nft_run(void) { return RB_NFT_RUN; }
extern "C" uint32_t rb_nft_block(void) { return RB_NFT_BLOCK; }
extern "C" uint32_t rb_nft_fix(void) { return RB_NFT_FIX; }

__device__ __forceinline__ uint32_t rb_ndigits10(uint32_t v) { return rb_ndigits(v) + (v >= 1000000000u ? 1u : 0u); }

// the nd decimal digits of v, the last one at e[-1] (nd = rb_ndigits10(v)): one predicated byte store per digit, no division
__device__ __forceinline__ void rb_put_dec(uint8_t *e, uint32_t v, uint32_t nd) {
    const bool big = v >= 10000u;
    uint32_t rest = 0;
    if (big) {
        rest = (uint32_t)(((uint64_t)v * 3518437209ull) >> 45); // v / 10000 (exact for 32-bit v)
        v -= rest * 10000u;
    }
    const uint32_t d4 = rb_digits4(v) | 0x30303030u;
    e[-1] = (uint8_t)d4;
    if (nd > 1u) e[-2] = (uint8_t)(d4 >> 8);
    if (nd > 2u) e[-3] = (uint8_t)(d4 >> 16);
    if (nd > 3u) e[-4] = (uint8_t)(d4 >> 24);
    if (big) { // digits 4..9 (rest < 429497)
        const uint32_t top = (uint32_t)(((uint64_t)rest * 3518437209ull) >> 45); // the ninth and tenth digit (0..42)
        const uint32_t e4 = rb_digits4(rest - top * 10000u) | 0x30303030u;
        e[-5] = (uint8_t)e4;
        if (nd > 5u) e[-6] = (uint8_t)(e4 >> 8);
        if (nd > 6u) e[-7] = (uint8_t)(e4 >> 16);
        if (nd > 7u) e[-8] = (uint8_t)(e4 >> 24);
        const uint32_t t10 = (top * 103u) >> 10; // top / 10 (exact below 179)
        if (nd > 8u) e[-9] = (uint8_t)(48u + top - t10 * 10u);
        if (nd > 9u) e[-10] = (uint8_t)(48u + t10);
    }
}

// what the wavefront wrote to LDS is there for all its lanes, and the other way round
__device__ __forceinline__ void rb_nft_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <bool FILL>
__global__ __launch_bounds__(256) void rb_k_nft(rb_nft_params p) {
    __shared__ __attribute__((aligned(16))) uint8_t stage_all[FILL ? 4 : 1][FILL ? RB_NFT_STAGE : 16];
    __shared__ uint8_t fix_all[FILL ? 4 : 1][FILL ? 512 : 4]; // the segment's prefix at [0, 255), its suffix at [256, 511)
    const uint32_t wib = rb_first(threadIdx.x >> 6);
    const uint64_t u64 = (uint64_t)blockIdx.x * 4u + wib;
    if (u64 >= p.n_units) return;
    const uint32_t u = (uint32_t)u64;
    const uint32_t lane = (uint32_t)rb_lane();
    // the segment of this run: the last one whose first run is not behind u (an empty segment has no run)
    uint32_t lo = 0, hi = (uint32_t)p.n_seg;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (rb_first(p.unit0[mid]) <= u) lo = mid; else hi = mid;
    }
    const uint32_t s = lo;
    const rb_nft_seg sg = p.seg[s];
    const uint32_t k0 = (u - rb_first(p.unit0[s])) * RB_NFT_RUN;
    const uint32_t n_seg_pos = rb_first(sg.n);
    const uint32_t nrun = n_seg_pos - k0 < RB_NFT_RUN ? n_seg_pos - k0 : RB_NFT_RUN; // (k0 < n: the run exists)
    const uint32_t pos0 = rb_first(sg.pos) + k0;
    const uint4 *__restrict__ src = reinterpret_cast<const uint4 *>(p.counts) + (rb_first64(sg.cnt) + k0);
    const bool small = p.mode == RB_NFT_SMALL;
    const uint32_t pre_len = small ? 0u : rb_first(sg.pre_len), suf_len = small ? 0u : rb_first(sg.suf_len);

    uint8_t *stg = stage_all[wib];
    uint8_t *fix = fix_all[wib];
    uint64_t gbase = 0;            // the text byte that byte 0 of the stage stands for (16-byte aligned)
    uint32_t have = 0, own_from = 0; // bytes [own_from, have) of the stage are this run's and not yet stored
    if (FILL) {
        for (uint32_t j = lane; j < pre_len; j += 64u) fix[j] = p.strings[sg.pre_off + j];
        for (uint32_t j = lane; j < suf_len; j += 64u) fix[256u + j] = p.strings[sg.suf_off + j];
        const uint64_t out = rb_first64(p.unit_off[u]);
        have = own_from = (uint32_t)(out & 15u);
        gbase = out - have;
        rb_nft_sync();
    }
    uint64_t bytes = 0;
    uint32_t lines = 0, first = ~0u;
    for (uint32_t s0 = 0; s0 < nrun; s0 += RB_NFT_STEP) {
        const uint32_t k = s0 + lane;
        uint4 c = make_uint4(0u, 0u, 0u, 0u);
        if (k < nrun) c = src[k];
        const bool covered = (c.x & RB_NF_COVERED) != 0u;
        const uint32_t pp = pos0 + k, pp1 = pp + 1u; // (the end column wraps at 2^32, as the reference's u32 does)
        uint32_t a = c.x & ~RB_NF_COVERED, b = c.y;
        if (small) { // the largest and the second largest of the four
            const uint32_t h0 = a > c.y ? a : c.y, l0 = a > c.y ? c.y : a, h1 = c.z > c.w ? c.z : c.w, l1 = c.z > c.w ? c.w : c.z;
            const uint32_t mx = h0 > h1 ? h0 : h1, other = h0 > h1 ? h1 : h0, lmax = l0 > l1 ? l0 : l1;
            a = mx, b = other > lmax ? other : lmax;
        }
        const uint32_t nd_a = rb_ndigits10(a), nd_b = rb_ndigits10(b);
        uint32_t nd_p = 0, nd_q = 0, nd_g = 0, nd_t = 0, len;
        if (small) {
            len = nd_a + nd_b + 2u;
        } else {
            nd_p = rb_ndigits10(pp), nd_q = rb_ndigits10(pp1), nd_g = rb_ndigits10(c.z), nd_t = rb_ndigits10(c.w);
            len = pre_len + nd_p + nd_q + nd_a + nd_b + nd_g + nd_t + 5u + suf_len; // (five TABs of its own)
        }
        if (!covered) len = 0u;
        const unsigned long long cov = rb_ballot(covered);
        const uint32_t incl = rb_wave_scan_incl(len);
        const uint32_t total = rb_readlane<uint32_t>(incl, 63);
        bytes += total;
        if (!FILL) {
            lines += (uint32_t)__builtin_popcountll(cov);
            if (first == ~0u && cov) first = s0 + (uint32_t)__builtin_ctzll(cov);
            continue;
        }
        // the lines of the step, as many at a time as the stage holds (all of them, unless the prefixes and suffixes are long)
        const uint32_t excl = incl - len;
        for (uint32_t base = 0; base < total;) {
            const bool in = len != 0u && excl >= base && have + (incl - base) <= RB_NFT_STAGE;
            const unsigned long long m = rb_ballot(in); // (never empty: the first line behind base fits)
            const uint32_t round_end = rb_readlane<uint32_t>(incl, 63 - (int)__builtin_clzll(m));
            if (in) {
                uint8_t *d = stg + have + (excl - base);
                if (small) {
                    d += nd_a;
                    rb_put_dec(d, a, nd_a);
                    *d++ = (uint8_t)'\t';
                    d += nd_b;
                    rb_put_dec(d, b, nd_b);
                    *d = (uint8_t)'\n';
                } else {
                    for (uint32_t j = 0; j < pre_len; j++) d[j] = fix[j];
                    d += pre_len + nd_p;
                    rb_put_dec(d, pp, nd_p);
                    *d++ = (uint8_t)'\t';
                    d += nd_q;
                    rb_put_dec(d, pp1, nd_q);
                    *d++ = (uint8_t)'\t';
                    d += nd_a;
                    rb_put_dec(d, a, nd_a);
                    *d++ = (uint8_t)'\t';
                    d += nd_b;
                    rb_put_dec(d, b, nd_b);
                    *d++ = (uint8_t)'\t';
                    d += nd_g;
                    rb_put_dec(d, c.z, nd_g);
                    *d++ = (uint8_t)'\t';
                    d += nd_t;
                    rb_put_dec(d, c.w, nd_t);
                    for (uint32_t j = 0; j < suf_len; j++) d[j] = fix[256u + j];
                }
            }
            rb_nft_sync();
            const uint32_t end = have + (round_end - base); // stage bytes [own_from, end) are waiting
            const uint32_t b16 = end & ~15u;
            if (b16) { // whole groups [a16, b16) leave wide; a first group shared with the run in front leaves byte by byte
                const uint32_t a16 = own_from ? 16u : 0u;
                if (own_from && lane >= own_from && lane < 16u && gbase + lane < p.text_cap) p.text[gbase + lane] = stg[lane];
                for (uint32_t g = a16 + 16u * lane; g < b16; g += 16u * 64u)
                    if (gbase + g + 16u <= p.text_cap) *reinterpret_cast<uint4 *>(p.text + gbase + g) = *reinterpret_cast<const uint4 *>(stg + g);
                const uint32_t t = end - b16; // what is left becomes the head of the next round
                const uint8_t v = lane < t ? stg[b16 + lane] : (uint8_t)0;
                rb_nft_sync();
                if (lane < t) stg[lane] = v;
                gbase += b16, have = t, own_from = 0u;
                rb_nft_sync();
            } else {
                have = end;
            }
            base = round_end;
        }
    }
    if (FILL) { // the run's last bytes: a group its neighbour behind may share
        if (lane >= own_from && lane < have && gbase + lane < p.text_cap) p.text[gbase + lane] = stg[lane];
    } else if (lane == 0u) {
        p.unit_off[u] = bytes;
        if (lines) {
            atomicAdd((unsigned long long *)&p.seg_lines[s], (unsigned long long)lines);
            atomicMin((unsigned long long *)&p.seg_first[s], (unsigned long long)rb_first(sg.pos) + k0 + first);
        }
    }
}

// seg_text_off[s] = where the segment's first run starts (unit_off scanned; unit0[n_seg] = n_units, unit_off[n_units] = all bytes)
__global__ __launch_bounds__(256) void rb_k_nft_seg_off(rb_nft_params p) {
    const uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (s <= p.n_seg) p.seg_text_off[s] = p.unit_off[p.unit0[s]];
}

extern "C" hipError_t rb_launch_nft(const rb_nft_params *p, bool fill, hipStream_t stream) {
    if (p->n_units == 0) return hipSuccess;
    const unsigned blocks = (unsigned)((p->n_units + 3) / 4);
    if (fill) hipLaunchKernelGGL(rb_k_nft<true>, dim3(blocks), dim3(256), 0, stream, *p);
    else hipLaunchKernelGGL(rb_k_nft<false>, dim3(blocks), dim3(256), 0, stream, *p);
    return hipGetLastError();
}
extern "C" hipError_t rb_launch_nft_seg_off(const rb_nft_params *p, hipStream_t stream) {
    hipLaunchKernelGGL(rb_k_nft_seg_off, dim3((unsigned)((p->n_seg + 1 + 255) / 256)), dim3(256), 0, stream, *p);
    return hipGetLastError();
}
