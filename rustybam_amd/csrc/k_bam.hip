// k_bam.hip -- the records of an inflated BAM stream as the columns `rb stats` needs (gfx950, wave64): rb_dev_bam_records.
//
// Restates bam_core and the aux loop of cigar_stats_bam (host/rb_host.cpp): the fixed fields and their three refusals, the walk over the
// optional fields for the last MD:Z and the last CG:B,I, the long-CIGAR convention, and the record's CIGAR words -- which in BAM are
// the packed words of this library already, at whatever BYTE the name's length leaves them -- gathered into the aligned ops array.
//
// Shape.  Three steps on the stream, no atomic decides a place, so two calls write the same bytes:
//   rb_k_bam_peek  a record is a ROW of 16 lanes, four records to a wavefront.  The hop from field to field is uniform within the row
//                  (every lane reads the same head: tag, type, and for B the subtype and count); the search for the NUL of a Z / H
//                  value is the row's work: 16 bytes per lane and step, a SWAR test for a zero byte, one ballot.  A record whose aux
//                  area is longer than RB_BAM_AUX_ROW_MAX bytes is left out of the row form and walked afterwards by the whole
//                  wavefront (1 KiB per step), so a 1 MiB MD costs its bytes and not a loop in one lane.  Writes every column, the
//                  record's op count into op_off[r] and the place of its words (in the record or in the CG tag) into scratch.
//   the device-wide exclusive scan of op_off (the three small launches every scan of this library takes).
//   rb_k_bam_copy  the gather, shaped as rb_k_rtb_fill (k_rows_batch.hip): a row per record, RB_BAM_COPY_ROW_STEP = 64 ops per step,
//                  CIGARs of more than RB_BAM_COPY_ROW_MAX ops by the wavefront afterwards.  The source is read in whole aligned
//                  16-byte groups; a lane that holds source group G builds DESTINATION group G from its own four words and the four of
//                  the lane in front of it (DPP; a register carries them across steps): with sh = (destination - source) mod 16
//                  BYTES, destination group G is source bytes 16 G - sh .. 16 G + 15 - sh, five consecutive words of the eight funnelled
//                  by v_alignbyte.  Interior groups leave as one aligned dwordx4, a CIGAR's first and last group word by word.
//
// Memory.  Only aligned dwords / 16-byte groups that hold at least one byte of the record are loaded (data is 16-byte aligned and
// readable to the next multiple of 16 behind the last record).  Algorithmic bytes: 36 B of fixed fields + the name's last byte + the
// aux area once per record, 4 B per op read and 4 B written, 12 B of rec_off / rec_len in and 62 B of columns, count and place out.
#include "rb_device.h"
#include "rb_launch.h"

#define RB_BAM_AUX_ROW_STEP 256u   // bytes per step of a row's NUL search
#define RB_BAM_AUX_WAVE_STEP 1024u // ... of the wavefront's
#ifndef RB_BAM_AUX_ROW_MAX
#define RB_BAM_AUX_ROW_MAX 16384u  // aux areas of more bytes than this take the wavefront form: with four equal records to a wavefront rows win up to 16384, a tie at 65536 (profiles/bam_stats_summary.md); above it the wavefront bounds what one long record among short ones costs
#endif
#define RB_BAM_COPY_ROW_STEP 64u   // ops per step of a row of 16 lanes (one 16-byte group per lane)
#define RB_BAM_COPY_WAVE_STEP 256u // ops per step of the whole wavefront (long CIGARs)
#ifndef RB_BAM_COPY_ROW_MAX
#define RB_BAM_COPY_ROW_MAX 4096u  // CIGARs of more ops than this take the wavefront form (rb_k_rtb_fill's line)
#endif
#define RB_BAM_COPY_BATCH 4        // steps whose loads are in flight together

extern "C" uint32_t rb_bam_aux_row_step(void) { return RB_BAM_AUX_ROW_STEP; }
extern "C" uint32_t rb_bam_aux_row_max(void) { return RB_BAM_AUX_ROW_MAX; }
extern "C" uint32_t rb_bam_aux_wave_step(void) { return RB_BAM_AUX_WAVE_STEP; }
extern "C" uint32_t rb_bam_copy_row_step(void) { return RB_BAM_COPY_ROW_STEP; }
extern "C" uint32_t rb_bam_copy_row_max(void) { return RB_BAM_COPY_ROW_MAX; }
extern "C" uint32_t rb_bam_copy_wave_step(void) { return RB_BAM_COPY_WAVE_STEP; }

// bit i = byte i of the 16 is zero (exact per byte: no borrow runs from one byte into the next)
__device__ __forceinline__ uint32_t rb_bam_zero_map(const uint4 v) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t m = 0u;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        uint32_t t = ~(((w[j] & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | w[j] | 0x7F7F7F7Fu); // bit 7 of every zero byte
        t >>= 7;
        t |= t >> 7;
        t |= t >> 14;
        m |= (t & 15u) << (4 * j);
    }
    return m;
}

struct rb_bam_aux {
    uint32_t has_md, has_cg, cg_n;
    uint64_t md_off, md_end, cg_off; // places in data
};

// The aux walk of one record by W lanes (16: a row, every row of the wavefront its own record; 64: the wavefront): the record's bytes
// are data[R .. R + bs), its aux area starts at R + p0.  Every lane of the wavefront runs every turn of the loop (the ballots need them
// all); what a row does in a turn depends on values that are the same in its 16 lanes.  A turn: the rows that stand at a field read its
// head and step over it -- or, at a Z / H value, start a search --, then every searching row looks at its next 2 * 16 W bytes.
template <int W>
__device__ __forceinline__ void rb_bam_aux_walk(const uint8_t *data, const uint64_t R, const uint64_t p0, const uint64_t bs, const bool take, const int lane,
                                                rb_bam_aux &o) {
    static_assert((W == 16 && 16 * W == RB_BAM_AUX_ROW_STEP) || (W == 64 && 16 * W == RB_BAM_AUX_WAVE_STEP), "a step is one 16-byte load per lane");
    const uint32_t gl = (uint32_t)lane & (uint32_t)(W - 1);
    const uint32_t gbase = (uint32_t)lane & ~(uint32_t)(W - 1);
    const uint64_t E = R + bs; // the record's end in data
    uint64_t p = p0;           // offset in the record of the next field
    bool go = take, searching = false, is_md = false;
    uint64_t v0 = 0, c = 0; // the value's first byte, the aligned place the search has reached (both in data)
    while (rb_ballot(go) != 0ull) {
        if (go && !searching) {
            if (p + 3u > bs) {
                go = false;
            } else {
                const uint64_t left = bs - p;
                const uint64_t h = rb_bam_bytes(data, R + p, left < 8u ? (uint32_t)left : 8u); // tag, type; of a B: subtype, count
                const uint32_t tag = (uint32_t)h & 0xFFFFu, ty = ((uint32_t)h >> 16) & 0xFFu, sub = (uint32_t)h >> 24, cnt = (uint32_t)(h >> 32);
                p += 3u;
                if (ty == 'A' || ty == 'c' || ty == 'C') p += 1u;
                else if (ty == 's' || ty == 'S') p += 2u;
                else if (ty == 'i' || ty == 'I' || ty == 'f') p += 4u;
                else if (ty == 'Z' || ty == 'H') {
                    searching = true;
                    is_md = tag == ((uint32_t)'M' | ((uint32_t)'D' << 8)) && ty == 'Z';
                    v0 = R + p, c = v0 & ~15ull;
                } else if (ty == 'B') {
                    const uint32_t es = (sub == 'c' || sub == 'C') ? 1u : ((sub == 's' || sub == 'S') ? 2u : 4u);
                    const uint64_t e = p + 5u + (uint64_t)es * cnt;
                    if (p + 5u > bs || e > bs) { // (a head or an array that runs past the record: the walk stops, as htslib's does)
                        go = false;
                    } else {
                        if (tag == ((uint32_t)'C' | ((uint32_t)'G' << 8)) && sub == 'I') o.has_cg = 1u, o.cg_off = R + p + 5u, o.cg_n = cnt;
                        p = e;
                    }
                } else {
                    go = false;
                }
            }
        }
        if (rb_ballot(go && searching) == 0ull) continue; // (uniform)
        const bool s = go && searching;
        uint32_t Z[2];
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const uint64_t la = c + (uint64_t)j * (16u * W) + gl * 16u;
            const bool ld = s && la < E; // (la + 16 > v0 > R: the group holds a byte of the record)
            uint4 v = make_uint4(~0u, ~0u, ~0u, ~0u);
            if (ld) v = *reinterpret_cast<const uint4 *>(data + la);
            const uint32_t fv = v0 > la ? (v0 - la < 16u ? (uint32_t)(v0 - la) : 16u) : 0u; // bytes [fv, ev) of the group belong to the value
            const uint32_t ev = ld ? (E - la < 16u ? (uint32_t)(E - la) : 16u) : 0u;
            Z[j] = rb_bam_zero_map(v) & ((1u << ev) - 1u) & ~((1u << fv) - 1u);
        }
        const unsigned long long B0 = rb_ballot(Z[0] != 0u), B1 = rb_ballot(Z[1] != 0u);
        const uint32_t g0 = W == 16 ? (uint32_t)(B0 >> gbase) & 0xFFFFu : 0u, g1 = W == 16 ? (uint32_t)(B1 >> gbase) & 0xFFFFu : 0u;
        const bool hit0 = W == 16 ? g0 != 0u : B0 != 0ull, hit1 = W == 16 ? g1 != 0u : B1 != 0ull;
        uint32_t fl; // the first lane of the group that holds a NUL
        if (W == 16) fl = (uint32_t)__builtin_ctz((hit0 ? g0 : g1) | 0x10000u) & 15u;
        else fl = (uint32_t)__builtin_ctzll((hit0 ? B0 : B1) | (1ull << 63));
        const uint32_t zf = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((gbase + fl) << 2), (int)(hit0 ? Z[0] : Z[1]));
        if (s) {
            uint64_t end = 0;
            bool done = true;
            if (hit0 || hit1) end = c + (hit0 ? 0u : 16u * W) + fl * 16u + (uint32_t)__builtin_ctz(zf | 0x10000u);
            else if (c + 2u * (16u * W) >= E) end = E; // (no NUL: the value runs to the record's end)
            else done = false, c += 2u * (16u * W);
            if (done) {
                if (is_md) o.has_md = 1u, o.md_off = v0, o.md_end = end;
                p = end - R + 1u;
                searching = false;
            }
        }
    }
}

__global__ __launch_bounds__(256) void rb_k_bam_peek(rb_bam_params p) {
    const int lane = rb_lane();
    const uint32_t gl = (uint32_t)lane & 15u;
    const uint64_t k0 = ((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6)) * 4u; // the wavefront's first record
    const uint64_t k = k0 + ((uint32_t)lane >> 4);
    const bool live = k < p.n;
    uint64_t R = 0, bs = 0;
    if (live) R = p.rec_off[k], bs = p.rec_len[k];
    uint32_t st = RB_BAM_OK, l_rn = 0, n_cig = 0, flag = 0, l_seq = 0;
    int32_t tid = 0, pos = 0;
    uint64_t need = 0;
    if (live && bs < 32u) st = RB_BAM_SHORT_BLOCK;
    if (live && st == RB_BAM_OK) {
        const uint64_t f0 = rb_bam_bytes(p.data, R, 8u), f1 = rb_bam_bytes(p.data, R + 8u, 8u), f2 = rb_bam_bytes(p.data, R + 16u, 4u);
        tid = (int32_t)(uint32_t)f0, pos = (int32_t)(uint32_t)(f0 >> 32);
        l_rn = (uint32_t)f1 & 0xFFu, n_cig = (uint32_t)(f1 >> 32) & 0xFFFFu, flag = (uint32_t)(f1 >> 48), l_seq = (uint32_t)f2;
        need = 32ull + l_rn + 4ull * n_cig + ((uint64_t)l_seq + 1u) / 2u + l_seq;
        if (need > bs) st = RB_BAM_NO_FIT;
        else if (l_rn == 0u || (rb_bam_bytes(p.data, R + 31u + l_rn, 1u) & 0xFFu) != 0u) st = RB_BAM_BAD_NAME;
    }
    const bool ok = live && st == RB_BAM_OK;
    const bool walk = ok && !(flag & 4u);
    const bool is_long = walk && bs - need > (uint64_t)RB_BAM_AUX_ROW_MAX;
    uint32_t first = 0u; // the first in-record CIGAR word (the long-CIGAR convention looks at it)
    if (walk && n_cig) first = (uint32_t)rb_bam_bytes(p.data, R + 32u + l_rn, 4u);
    rb_bam_aux a;
    a.has_md = a.has_cg = a.cg_n = 0u, a.md_off = a.md_end = a.cg_off = 0ull;
    rb_bam_aux_walk<16>(p.data, R, need, bs, walk && !is_long, lane, a);
    // ---- the long aux areas of these four records, one after the other, by the whole wavefront ----
    unsigned long long todo = rb_ballot(is_long && gl == 0u);
    while (todo) {
        const int b = __builtin_ctzll(todo);
        todo &= todo - 1ull;
        const uint64_t lR = rb_readlane<uint64_t>(R, b), lbs = rb_readlane<uint64_t>(bs, b), lneed = rb_readlane<uint64_t>(need, b);
        rb_bam_aux al;
        al.has_md = al.has_cg = al.cg_n = 0u, al.md_off = al.md_end = al.cg_off = 0ull;
        rb_bam_aux_walk<64>(p.data, lR, lneed, lbs, true, lane, al);
        if (((uint32_t)lane >> 4) == ((uint32_t)b >> 4)) a = al;
    }
    if (!live || gl != 0u) return;
    uint64_t src = 0, cnt = 0;
    if (!ok) tid = pos = 0, flag = l_seq = 0u;
    if (walk) {
        src = R + 32u + l_rn, cnt = n_cig;
        if (a.has_cg && n_cig >= 1u && (first & 15u) == (uint32_t)RB_OP_S && (first >> 4) == l_seq) src = a.cg_off, cnt = a.cg_n;
    }
    p.tid[k] = tid;
    p.pos[k] = (int64_t)pos;
    p.flag[k] = flag;
    p.l_seq[k] = l_seq;
    p.has_md[k] = (uint8_t)a.has_md;
    p.md_off[k] = a.md_off;
    p.md_end[k] = a.md_end;
    p.status[k] = (uint8_t)st;
    p.op_off[k] = cnt;
    p.src[k] = src;
}

// ---- the gather -------------------------------------------------------------------------------------
struct rb_bam_cigar {
    const uint8_t *gsrc; // the aligned group that holds the first byte of the words
    uint32_t head;       // bytes of that group in front of it (0 .. 15)
    uint32_t n;          // words
};

// One CIGAR by W lanes.  d0 = index in ops of its first word.  Coordinates in BYTES: e = source coordinate (counted from gsrc) + sh, so
// that e and the destination's byte offset agree mod 16; the words are e in [e0, e1), destination group G = e in [16 G, 16 G + 16)
// lies at byte dbase + 16 G of ops.
template <int W>
__device__ __forceinline__ void rb_bam_copy_walk(const rb_bam_cigar &c, const bool take, const uint64_t d0, uint32_t *ops, const uint64_t ops_cap, const int lane) {
    static_assert((W == 16 && 4 * W == RB_BAM_COPY_ROW_STEP) || (W == 64 && 4 * W == RB_BAM_COPY_WAVE_STEP), "a step is one 16-byte group per lane");
    const uint32_t gl = (uint32_t)lane & (uint32_t)(W - 1);
    const uint32_t n = c.n;
    const uint32_t sh = (((uint32_t)d0 << 2) - c.head) & 15u;
    const uint64_t e0 = (uint64_t)c.head + sh, e1 = e0 + 4ull * n;
    const int64_t dbase = (int64_t)(d0 << 2) - (int64_t)e0; // a multiple of 16 (-16 at the least)
    const bool live = take && n != 0u;
    const uint32_t n_steps = live ? (uint32_t)((e1 + (16u * W - 1u)) / (16u * W)) : 0u;
    const uint64_t last_off = live ? (((uint64_t)c.head + 4ull * n - 1u) & ~15ull) : 0ull;
    uint32_t w_steps = n_steps; // the wavefront's steps: the longest of its CIGARs
    if (W == 16) {
#pragma unroll
        for (int off = 16; off < 64; off <<= 1) {
            const uint32_t o = (uint32_t)__shfl_xor((int)w_steps, off, 64);
            w_steps = w_steps > o ? w_steps : o;
        }
    }
    w_steps = rb_first(w_steps);
    // which five of the eight words (the group in front, mine) hold destination group G, and the byte they are funnelled by
    const uint32_t wbase = ((sh & 3u) ? 3u : 4u) - (sh >> 2); // 0 .. 4
    const uint32_t fun = (4u - (sh & 3u)) & 3u;
    uint32_t cx = 0u, cy = 0u, cz = 0u, cw = 0u; // the group in front of this step's first one
    for (uint32_t b0 = 0; b0 < w_steps; b0 += RB_BAM_COPY_BATCH) {
        uint4 pf[RB_BAM_COPY_BATCH];
#pragma unroll
        for (int s = 0; s < RB_BAM_COPY_BATCH; s++) {
            uint64_t off = (uint64_t)(b0 + (uint32_t)s) * (16u * W) + gl * 16u;
            off = off < last_off ? off : last_off; // (past the last group: that group again; its bytes are not stored)
            pf[s] = live ? *reinterpret_cast<const uint4 *>(c.gsrc + off) : make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (int s = 0; s < RB_BAM_COPY_BATCH; s++) {
            const uint32_t st = b0 + (uint32_t)s;
            if (st >= w_steps) break; // (uniform)
            const uint4 v = pf[s];
            uint32_t px, py, pz, pw; // the source group in front of mine
            if (W == 16) {
                px = (uint32_t)__builtin_amdgcn_update_dpp((int)cx, (int)v.x, RB_DPP_ROW_SHR(1), 0xf, 0xf, false);
                py = (uint32_t)__builtin_amdgcn_update_dpp((int)cy, (int)v.y, RB_DPP_ROW_SHR(1), 0xf, 0xf, false);
                pz = (uint32_t)__builtin_amdgcn_update_dpp((int)cz, (int)v.z, RB_DPP_ROW_SHR(1), 0xf, 0xf, false);
                pw = (uint32_t)__builtin_amdgcn_update_dpp((int)cw, (int)v.w, RB_DPP_ROW_SHR(1), 0xf, 0xf, false);
                cx = rb_row_last(v.x), cy = rb_row_last(v.y), cz = rb_row_last(v.z), cw = rb_row_last(v.w);
            } else {
                px = rb_prev_lane(v.x, cx), py = rb_prev_lane(v.y, cy), pz = rb_prev_lane(v.z, cz), pw = rb_prev_lane(v.w, cw);
                cx = rb_readlane<uint32_t>(v.x, 63), cy = rb_readlane<uint32_t>(v.y, 63), cz = rb_readlane<uint32_t>(v.z, 63), cw = rb_readlane<uint32_t>(v.w, 63);
            }
            if (st < n_steps) { // (uniform over the W lanes: a row whose CIGAR has ended sits the step out)
                uint32_t t[5]; // words wbase .. wbase + 4 of px py pz pw v.x v.y v.z v.w (the ninth is never looked at: fun == 0 there)
                t[0] = wbase == 0u ? px : wbase == 1u ? py : wbase == 2u ? pz : wbase == 3u ? pw : v.x;
                t[1] = wbase == 0u ? py : wbase == 1u ? pz : wbase == 2u ? pw : wbase == 3u ? v.x : v.y;
                t[2] = wbase == 0u ? pz : wbase == 1u ? pw : wbase == 2u ? v.x : wbase == 3u ? v.y : v.z;
                t[3] = wbase == 0u ? pw : wbase == 1u ? v.x : wbase == 2u ? v.y : wbase == 3u ? v.z : v.w;
                t[4] = wbase == 0u ? v.x : wbase == 1u ? v.y : wbase == 2u ? v.z : wbase == 3u ? v.w : 0u;
                uint32_t o[4];
#pragma unroll
                for (int q = 0; q < 4; q++) o[q] = __builtin_amdgcn_alignbyte(t[q + 1], t[q], fun);
                const uint64_t eg = (uint64_t)st * (16u * W) + gl * 16u; // e of o[0]
                const int64_t dg = (dbase + (int64_t)eg) >> 2;           // index of o[0] in ops
                if (eg >= e0 && eg + 16u <= e1 && (uint64_t)dg + 4u <= ops_cap) { // a group that is the CIGAR's alone
                    *reinterpret_cast<uint4 *>(ops + dg) = make_uint4(o[0], o[1], o[2], o[3]);
                } else {
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const uint64_t e = eg + 4u * (uint32_t)q;
                        if (e < e0 || e >= e1) continue;
                        if ((uint64_t)(dg + q) < ops_cap) ops[dg + q] = o[q];
                    }
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void rb_k_bam_copy(rb_bam_params p) {
    const int lane = rb_lane();
    const uint32_t gl = (uint32_t)lane & 15u;
    const uint64_t k0 = ((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6)) * 4u; // the wavefront's first record
    const uint64_t k = k0 + ((uint32_t)lane >> 4);
    const bool in = k < p.n;
    rb_bam_cigar c;
    c.gsrc = p.data, c.head = 0u, c.n = 0u;
    uint64_t d0 = 0;
    if (in) {
        const uint64_t src = p.src[k];
        d0 = p.op_off[k]; // (scanned: where the record's ops go)
        c.n = (uint32_t)(p.op_off[k + 1] - d0);
        c.head = (uint32_t)src & 15u;
        c.gsrc = p.data + (src & ~15ull);
    }
    const bool is_long = in && c.n > RB_BAM_COPY_ROW_MAX;
    rb_bam_copy_walk<16>(c, in && !is_long, d0, p.ops, p.ops_cap, lane);
    // ---- the long CIGARs of these four records, one after the other, by the whole wavefront ----
    unsigned long long todo = rb_ballot(is_long && gl == 0u);
    while (todo) {
        const uint32_t b = (uint32_t)__builtin_ctzll(todo);
        todo &= todo - 1ull;
        const uint64_t kk = k0 + (b >> 4);
        const uint64_t src = rb_first64(p.src[kk]), l0 = rb_first64(p.op_off[kk]), l1 = rb_first64(p.op_off[kk + 1]);
        rb_bam_cigar cl;
        cl.n = (uint32_t)(l1 - l0), cl.head = (uint32_t)src & 15u, cl.gsrc = p.data + (src & ~15ull);
        rb_bam_copy_walk<64>(cl, true, l0, p.ops, p.ops_cap, lane);
    }
}

extern "C" hipError_t rb_launch_bam_peek(const rb_bam_params *p, hipStream_t stream) {
    if (p->n == 0) return hipSuccess;
    hipLaunchKernelGGL(rb_k_bam_peek, dim3((unsigned)((p->n + 15) / 16)), dim3(256), 0, stream, *p);
    return hipGetLastError();
}
extern "C" hipError_t rb_launch_bam_copy(const rb_bam_params *p, hipStream_t stream) {
    if (p->n == 0) return hipSuccess;
    hipLaunchKernelGGL(rb_k_bam_copy, dim3((unsigned)((p->n + 15) / 16)), dim3(256), 0, stream, *p);
    return hipGetLastError();
}
