// rb_pair.h -- what a trim-paf pair kernel is, stated once for the three device forms behind rb_launch_overlap_split: the row form
// (k_trim4.hip, four pairs per wavefront), the wave form (k_trim.hip, a wavefront per pair with larger regions) and the serial kernel
// (k_trim.hip, a thread per pair).  The two staged forms share how a pair is opened and declined, the positions a cut is made of and
// truncate_record_by_query itself (rb_pair_clip); what differs -- how a record's region is staged and searched -- each form keeps, and
// hands to the clip as a small "region" type.
#pragma once
#include "rb_trim.h"

__device__ __forceinline__ rb_pair_row rb_pair_row_empty() {
    rb_pair_row w;
    w.split_idx = 0;
    w.split_score = 0;
    w.status = RB_ST_OK;
    w._pad = 0; // (diagnostic: low half -- a staged form that cuts the pair leaves 1, the serial kernel 0; high half -- the row kernel leaves 1)
    for (int s = 0; s < 2; s++) {
        w.t_st[s] = w.t_en[s] = w.q_st[s] = w.q_en[s] = 0;
        w.nmatch[s] = w.aln_len[s] = 0;
        w.out_off[s] = 0;
        w.out_n[s] = 0;
    }
    return w;
}

struct rb_ppos { // an op (i = n: none), its word, and the exclusive prefix of the searched quantity at it
    uint32_t i, w, pre;
};
struct rb_pend { // a unit of the record: its index, the op that holds it, and the prefixes before that op
    uint32_t k;    // unit
    rb_ppos o;     // op, its word, units before it
    uint32_t R, Q; // reference / query bases before the op
};
struct rb_pcut { // the two end words of a clip (absolute indices into the ops array), written in place once BOTH clips of the pair stand
    uint64_t at_first, at_last;
    uint32_t w_first, w_last;
};
// A record of a pair as the staged forms see it: the part both share.  Only a REGION of the record -- ops [i0, i0 + m) -- is staged,
// with prefixes that are absolute (counted from the record's first op); rb_wrec / rb_qrec add where their region lives.
struct rb_prec {
    const uint32_t *ops; // the record's kept ops, in memory
    uint32_t n;          // how many
    uint32_t i0, m;      // the staged region
    uint64_t t_st, t_en, q_st, q_en;
    bool minus;
    bool bad;               // a question the region cannot answer: the pair goes to the kernels behind this one
    uint32_t N, Qtot, Rtot; // totals of the whole record (units from the norm row, bases from the coordinates)
    uint32_t xa, xb;        // query offsets, in the record's op order, of the overlap's first and last base
};

// list a pair for the kernels behind this one (why: diagnostics, RB_DEBUG_TRIM_NO_SERIAL; whoever does the pair rewrites the whole row)
__device__ __forceinline__ void rb_pair_pending(const rb_trim_params &p, uint64_t pi, bool lead, uint32_t why) {
    if (lead) {
        if (p.list_declined) p.pend_list[atomicAdd(p.pend, 1ull)] = (uint32_t)pi; // (listed once: by the first attempt)
        p.rows[pi].status = RB_ST_PENDING_INTERNAL, p.rows[pi].split_idx = why;
    }
}

// Open pair pi: both records from their norm rows, the overlap [st_ovl, en_ovl) on the query (trim_overlap.rs:43-44) and where it lies
// in each record's op order.  Returns RB_PAIR_OPENED, RB_PAIR_CLOSED (a record the reference panics on: the row is written), or why the
// pair is declined -- 1: a record that is not regular, or a policy this instantiation does not serve (LEG serves the legacy one);
// 2: no overlap (the serial kernel says what the reference does) -- for the caller to list.  `lead`: the lane that writes for the pair.
#define RB_PAIR_OPENED 0u
#define RB_PAIR_CLOSED 0xFFFFFFFFu
template <bool LEG>
__device__ __forceinline__ uint32_t rb_pair_open(const rb_trim_params &p, uint64_t pi, bool lead, rb_pair_row &w, rb_prec &L, rb_prec &R, uint64_t *st_ovl,
                                                 uint64_t *en_ovl) {
    const uint32_t rl = p.left[pi], rr = p.right[pi];
    const rb_norm_row nl = p.norm[rl], nr = p.norm[rr];
    if (nl.status != RB_ST_OK || nr.status != RB_ST_OK) { // aligned_pairs() panics (paf.rs:273-274, :782)
        w.status = nl.status != RB_ST_OK ? nl.status : nr.status;
        if (lead) p.rows[pi] = w;
        return RB_PAIR_CLOSED;
    }
    if ((!LEG && p.policy == RB_BSEARCH_LEGACY) || !(nl.flags & RB_F_REGULAR) || !(nr.flags & RB_F_REGULAR) || nl.n_ops == 0 || nr.n_ops == 0) return 1u;
    L.ops = p.ops + p.op_off[rl] + nl.first_op, L.n = nl.n_ops;
    L.t_st = nl.t_st, L.t_en = nl.t_en, L.q_st = nl.q_st, L.q_en = nl.q_en, L.minus = p.strand[rl] == (uint8_t)'-';
    L.N = nl.aln_len, L.Qtot = (uint32_t)(nl.q_en - nl.q_st), L.Rtot = (uint32_t)(nl.t_en - nl.t_st), L.bad = false;
    R.ops = p.ops + p.op_off[rr] + nr.first_op, R.n = nr.n_ops;
    R.t_st = nr.t_st, R.t_en = nr.t_en, R.q_st = nr.q_st, R.q_en = nr.q_en, R.minus = p.strand[rr] == (uint8_t)'-';
    R.N = nr.aln_len, R.Qtot = (uint32_t)(nr.q_en - nr.q_st), R.Rtot = (uint32_t)(nr.t_en - nr.t_st), R.bad = false;
    const uint64_t st = L.q_st > R.q_st ? L.q_st : R.q_st, en = L.q_en < R.q_en ? L.q_en : R.q_en;
    *st_ovl = st, *en_ovl = en;
    if (en <= st || st < L.q_st || en > L.q_en || st < R.q_st || en > R.q_en) return 2u;
    L.xa = (uint32_t)(!L.minus ? st - L.q_st : L.q_en - en), L.xb = (uint32_t)(!L.minus ? en - 1 - L.q_st : L.q_en - 1 - st);
    R.xa = (uint32_t)(!R.minus ? st - R.q_st : R.q_en - en), R.xb = (uint32_t)(!R.minus ? en - 1 - R.q_st : R.q_en - 1 - st);
    return RB_PAIR_OPENED;
}

// both clips of an in-place cut stand: their end words, where they are (first before last: a one-op cut writes the same word twice)
__device__ __forceinline__ void rb_pair_write_cuts(uint32_t *ops, const rb_pcut &cl, const rb_pcut &cr) {
    ops[cl.at_first] = cl.w_first, ops[cl.at_last] = cl.w_last;
    ops[cr.at_first] = cr.w_first, ops[cr.at_last] = cr.w_last;
}

// truncate_record_by_query (paf.rs:785-823) on a staged regular record; same results as rb_clip_by_query (k_trim.hip).  One end of the
// new query range is the record's own end (trim_overlap.rs:77-78), the other lies in the staged region.  What the clip asks of the
// region, rg (a type of the form's own; k = index into the region, i = i0 + k = index into the record):
//   rg.word(k), rg.qpre(k)              the op word / the query bases before the op; k = m: the sentinel behind the region
//   rg.q_begin(), rg.q_end()            the query offsets where the region starts and ends
//   rg.first_word(), rg.second_word(), rg.last_word()   of the record
//   rg.find_q(x)                        the query op that holds query offset x (i = n: none in the region)
//   rg.units_before(i), rg.ref_before(i)
//   rg.behind_last_base<LEG>(o, u, om)  x is the last base of op o and om = o at unit u: move u (and om with it) to the unit of the D / N
//                                       run behind o that the search returns -- the run's last unit (modern policy) or the one the legacy
//                                       search probes first (LEG).  false: the region cannot say.  The one step the forms do differently.
//   rg.lane(), RG::WIDTH                this lane among the WIDTH lanes that work on the pair
// in_place: nothing is copied, the row points at the run of ops the clip keeps and `cut` holds its two end words for
// rb_pair_write_cuts (rec_base = where the record's kept ops begin in the ops array).  A clip the region cannot answer sets v.bad.
template <bool LEG, class RG>
__device__ __forceinline__ uint32_t rb_pair_clip(rb_prec &v, const RG &rg, uint64_t new_q_st, uint64_t new_q_en, uint32_t *out, rb_pair_row *row, int s,
                                                 uint64_t out_base, bool in_place, rb_pcut &cut, uint64_t rec_base) {
    if (!(new_q_st >= v.q_st) || !(new_q_en <= v.q_en) || new_q_en == 0) return RB_ST_PANIC_ASSERT; // :787-788
    if (new_q_en <= new_q_st) { // an empty range: the serial kernel says what the reference does with it
        v.bad = true;
        return RB_ST_OK;
    }
    const uint32_t n = v.n, N = v.N;
    // the match-type unit truncate_record_by_query ends up at for query position p: qpos_to_idx_match (paf.rs:564-590) = the last
    // unit whose qpos equals p (modern policy) or the one the legacy search probes first (LEG), then the nearest match-type unit in the
    // search direction
    auto resolve = [&](uint64_t p, bool search_up, rb_pend *e) -> bool {
        if (p < v.q_st || p >= v.q_en) return false;
        const uint32_t x = (uint32_t)(v.minus ? v.q_en - 1 - p : p - v.q_st);
        if (x < rg.q_begin() || x >= rg.q_end()) {
            // outside the region: only the record's own first / last query base is asked for there.  A regular record starts and
            // ends on a match op; its last base is its last unit, its first base its first unit unless that op has one base and a
            // D / N run behind it (the run repeats the position: left to the kernels behind this one)
            if (x == 0u) {
                const uint32_t w0 = rg.first_word();
                if (rb_len(w0) < 2u && n > 1u && !rb_in(RB_QRY_MASK, rb_opc(rg.second_word()))) return false;
                e->k = 0, e->o.i = 0, e->o.w = w0, e->o.pre = 0, e->R = 0, e->Q = 0;
                return true;
            }
            if (x + 1u == v.Qtot) {
                const uint32_t wl = rg.last_word(), len = rb_len(wl);
                e->k = N - 1u, e->o.i = n - 1u, e->o.w = wl, e->o.pre = N - len, e->R = v.Rtot - len, e->Q = v.Qtot - len;
                return true;
            }
            return false;
        }
        const rb_ppos o = rg.find_q(x);
        if (o.i >= n) return false;
        const uint32_t j = x - o.pre, len = rb_len(o.w);
        const uint32_t ub = rg.units_before(o.i);
        uint32_t u = ub + j;
        rb_ppos om; // the op that holds unit u
        om.i = o.i, om.w = o.w, om.pre = ub;
        // last base of the op: the D / N units behind it repeat its position
        if (j + 1u == len && !rg.template behind_last_base<LEG>(o, u, om)) return false;
        // nearest match-type unit, up (paf.rs:581-583) or down (:585-587)
        uint32_t km = u;
        if (!rb_in(RB_MATCH_MASK, rb_opc(om.w))) {
            if (search_up) {
                uint32_t uu = om.pre + rb_len(om.w), k2 = om.i - v.i0 + 1u;
                for (; k2 < v.m && !rb_in(RB_MATCH_MASK, rb_opc(rg.word(k2))); k2++) uu += rb_len(rg.word(k2));
                if (k2 >= v.m) return false; // (no match op behind it inside the region; at the record's end the reference panics: serial kernel)
                km = uu;
                om.i = v.i0 + k2, om.w = rg.word(k2), om.pre = uu;
            } else {
                uint32_t uu = om.pre, k2 = om.i - v.i0;
                bool got = false;
                while (k2 > 0u) {
                    k2--;
                    if (rb_in(RB_MATCH_MASK, rb_opc(rg.word(k2)))) {
                        got = true;
                        break;
                    }
                    uu -= rb_len(rg.word(k2));
                }
                if (!got) return false;
                km = uu - 1u;
                om.i = v.i0 + k2, om.w = rg.word(k2), om.pre = uu - rb_len(rg.word(k2));
            }
        }
        e->k = km, e->o = om, e->R = rg.ref_before(om.i), e->Q = rg.qpre(om.i - v.i0);
        return true;
    };
    rb_pend A, B; // paf.rs:792-796: the start searches up on '+' and down on '-', the end the other way
    if (!resolve(new_q_st, !v.minus, &A) || !resolve(new_q_en - 1, v.minus, &B)) {
        v.bad = true;
        return RB_ST_OK;
    }
    auto unit = [&](const rb_pend &e, uint64_t *tpos, uint64_t *qpos) { // both are match-type units
        const uint32_t off = e.k - e.o.pre;
        *tpos = v.t_st + e.R + off;
        *qpos = v.minus ? v.q_en - 1 - e.Q - off : v.q_st + e.Q + off;
    };
    uint64_t tp, qp_st, qp_en;
    unit(A, &tp, &qp_st);
    unit(B, &tp, &qp_en);
    const uint64_t nq_st = qp_st, nq_en = qp_en + 1;
    if (A.k > B.k) { // :799-801
        const rb_pend t = A;
        A = B;
        B = t;
    }
    uint64_t t0, t1, qd;
    unit(A, &t0, &qd);
    unit(B, &t1, &qd);
    const uint64_t nt_st = t0, nt_en = t1 + 1; // :802-803
    // subset_cigar + collapse (:807-808): ops ia..ib with the first / last length cut; adjacent ops differ, nothing merges; both ends
    // are match-type units, so the strip of :819-822 removes nothing.
    // The copy is only a copy.  check_integrity of the clipped record (:819-822) compares the sums of its ops with coordinates that were
    // derived from those very prefixes: for a regular record it cannot fail, and nmatch follows from the spans (a match-type op counts in
    // reference, query and units, an I in query and units, a D / N in reference and units, so matches = ref + query - units: the clip
    // kernel's identity).  Summing three 64-bit totals over every copied op was 470 of a pair's 2640 vector instructions in the wave form.
    const uint32_t ia = A.o.i, ib = B.o.i, cnt = ib - ia + 1;
    const uint32_t lf = cnt == 1 ? B.k - A.k + 1u : A.o.pre + rb_len(A.o.w) - A.k, ll = cnt == 1 ? lf : B.k - B.o.pre + 1u;
    cut.at_first = rec_base + ia, cut.at_last = rec_base + ib;
    cut.w_first = (lf << 4) | rb_opc(A.o.w), cut.w_last = (ll << 4) | rb_opc(B.o.w);
    if (in_place) {
        out_base = rec_base + ia;
    } else {
        for (uint32_t j = rg.lane(); j < cnt; j += RG::WIDTH) {
            const uint32_t wv = v.ops[ia + j];
            out[j] = j == 0 ? ((lf << 4) | rb_opc(wv)) : (j == cnt - 1 ? ((ll << 4) | rb_opc(wv)) : wv);
        }
    }
    // (what CAN fail is the query side: the new start and end are resolved independently -- up and down --, and when the end lands on
    //  a lower query position than the start the coordinates say end + 1 - start while the ops between the two units still hold
    //  |end - start| + 1 query bases: check_integrity's unwrap panics)
    if (nt_en < nt_st) return RB_ST_PANIC_INTEGRITY_T;
    if (qp_en < qp_st) return RB_ST_PANIC_INTEGRITY_Q;
    const uint32_t units = B.k - A.k + 1u;
    row->t_st[s] = nt_st;
    row->t_en[s] = nt_en;
    row->q_st[s] = nq_st;
    row->q_en[s] = nq_en;
    row->nmatch[s] = (uint32_t)((nt_en - nt_st) + (nq_en - nq_st) - units);
    row->aln_len[s] = units;
    row->out_off[s] = out_base;
    row->out_n[s] = cnt;
    return RB_ST_OK;
}
