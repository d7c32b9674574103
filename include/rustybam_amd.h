/*
 * rustybam_amd.h -- C ABI of the MI355X (gfx950) CIGAR-walk engine.
 *
 * Drop-in boundary for the per-record CIGAR walk of mrvollger/rustybam v0.1.33.  The
 * reference has no FFI seam; the entry points below are what a Rust host would bind with
 * `extern "C"` in place of the following calls (file:line into the reference's src/):
 *
 *   rb_dev_scan_records   <- PafRecord::check_integrity / infer_n_bases   paf.rs:825-857, :631-654
 *                            (called per record by Paf::from_file         paf.rs:70)
 *                            PafRecord::remove_trailing_indels            paf.rs:656-783
 *                            bamstats::add_stats_from_cigar/stats_from_paf bamstats.rs:107-154, :91-105
 *   rb_dev_liftover       <- liftover::trim_paf_by_rgns                   liftover.rs:134-167
 *                            (= trim_helper :107-132 + trim_paf_rec_to_rgn :17-105, which in turn
 *                             replace aligned_pairs paf.rs:501-538, tpos_to_idx(_match) :541-561,
 *                             subset_cigar/collapse_long_cigar :593-620, paf_overlaps_rgn :622-627)
 *   rb_dev_break          <- liftover::break_paf_on_indels                liftover.rs:182-226
 *   rb_dev_swap           <- paf::paf_swap_query_and_target               paf.rs:1050-1094
 *   rb_dev_overlap_split  <- trim_overlap::trim_overlapping_pafs          trim_overlap.rs:36-86
 *   rb_dev_trim_select    <- the pair scan / selection of Paf::overlapping_paf_recs   paf.rs:223-284
 *                            + PafRecord::truncate_record_by_query        paf.rs:785-823
 *                            (the pass / recursion driver Paf::overlapping_paf_recs, paf.rs:210-305, stays on the host)
 *   rb_dev_nucfreq        <- nucfreq::nucfreq / region_nucfreq            nucfreq.rs:61-95, :111-125
 *   rb_dev_largest        <- liftover --largest: sort_by id, group_by id, max_by_key     main.rs:200-208
 *   rb_dev_stats_rows     <- bamstats::stats_from_paf / add_stats_from_cigar              bamstats.rs:91-105, :107-154
 *                            + PafRecord::check_integrity (paf.rs:825-857) of every record that trim_paf_by_rgns /
 *                            break_paf_on_indels returned (the second command of `rb liftover .. | rb stats --paf`)
 *   rb_dev_parse_md       <- bamstats::parse_md_for_stats                                 bamstats.rs:48-79
 *   rb_dev_aln_stats      <- bamstats::cigar_stats minus the names: query span, strand flip, MD refinement   bamstats.rs:129-142, :190-207
 *   rb_dev_bam_records    <- what main.rs:60-77 takes from htslib's bam_read1 per record: fields, MD:Z, CIGAR (CG:B,I included)
 *
 * Conventions
 *   - Plain C types only.  Every `rb_dev_*` pointer argument is a DEVICE pointer (HBM) owned by
 *     the caller; the call enqueues kernels on the context's HIP stream and returns without
 *     synchronising.  `rb_host_*` take HOST pointers and do H2D / kernels / D2H themselves.
 *   - Return value: RB_OK (0) or a negative rb_error; no exceptions or unwinding cross the ABI.
 *     Where the reference would panic or silently drop a (record, window) pair the outcome is
 *     a per-record / per-hit `status` in the result rows (enum rb_status).
 *   - One context per host thread; a context pins one device and one stream.
 *   - The library never falls back to the CPU: without a usable gfx950 device every compute
 *     entry point fails with RB_E_NO_DEVICE.
 *
 * Data model (all little-endian, in HBM):
 *   ops[]      u32  packed BAM encoding  len << 4 | op   (M0 I1 D2 N3 S4 H5 P6 =7 X8); 16-byte aligned (128 is faster), and
 *              readable -- contents ignored -- up to the next multiple of 32 ops behind the last one.
 *              A length of 2^28 and more (rust-htslib's Cigar holds a u32; a chromosome-long `=` of a plant genome aligned to
 *              itself has one) takes TWO words: (len & (2^28 - 1)) << 4 | op, then the CONTINUATION word
 *              (len >> 28) << 4 | RB_OP_CONT.  Inputs may hold such pairs and outputs (out_ops) hold them wherever a clipped
 *              or merged op is that long; every count of "ops" in this interface (op_off, first_op, n_ops, lead_ops,
 *              trail_ops, out_n) counts WORDS.  A record with a continuation word is not "regular": it takes the general
 *              kernels (same results, slower).  A continuation word with no op in front of it is a word of an unknown code:
 *              it consumes nothing.
 *   op_off[]   u64  [n_rec + 1] exclusive prefix of ops-per-record
 *   t_st,t_en,q_st,q_en u64 [n_rec];  strand u8 ('+' / '-');  contig u32 (dense ids, host keeps names)
 *   windows: contig u32, st u64, en u64   [n_win]  in BED file order
 */
#ifndef RUSTYBAM_AMD_H
#define RUSTYBAM_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RB_ABI_VERSION 1

enum rb_op { RB_OP_M = 0, RB_OP_I = 1, RB_OP_D = 2, RB_OP_N = 3, RB_OP_S = 4, RB_OP_H = 5, RB_OP_P = 6, RB_OP_EQ = 7, RB_OP_X = 8,
             RB_OP_CONT = 14 /* continuation word: bits 28..31 of the length of the op in front of it (see "ops[]" above) */ };

typedef enum rb_error {
    RB_OK = 0,
    RB_E_INVALID = -1,   /* bad argument */
    RB_E_NO_DEVICE = -2, /* no gfx950 device / HIP runtime unusable: there is NO CPU fallback */
    RB_E_HIP = -3,       /* a HIP call failed; see rb_ctx_last_error */
    RB_E_CAPACITY = -4,  /* caller-provided output buffer too small; counters say what is needed */
    RB_E_NOMEM = -5
} rb_error;

/* Per-record and per-hit outcome.  0 = Some(record).  1..5 = the reference returns None (pair is
 * silently dropped).  >= 16 = the reference panics at the cited line. */
typedef enum rb_status {
    RB_ST_OK = 0,
    RB_ST_NONE_INDEL = 1,         /* liftover.rs:52-54   start_idx > end_idx                    */
    RB_ST_NONE_NOMATCH = 2,       /* liftover.rs:65-75                                          */
    RB_ST_NONE_EMPTY = 3,         /* liftover.rs:87-89                                          */
    RB_ST_NONE_INVERTED = 4,      /* liftover.rs:90-96                                          */
    RB_ST_NONE_INTEGRITY = 5,     /* liftover.rs:99-102                                         */
    RB_ST_PANIC_NOTFOUND = 16,    /* liftover.rs:31 / :42, paf.rs:792-793                       */
    RB_ST_PANIC_EMPTY_CIGAR = 17, /* paf.rs:663                                                 */
    RB_ST_PANIC_INTEGRITY_T = 18, /* paf.rs:827 through .unwrap() at paf.rs:70 / :782           */
    RB_ST_PANIC_INTEGRITY_Q = 19, /* paf.rs:839                                                 */
    RB_ST_PANIC_ALL_INDEL = 20,   /* paf.rs:757                                                 */
    RB_ST_PANIC_ASSERT = 21,      /* paf.rs:787-788                                             */
    RB_ST_PANIC_OVERFLOW = 22     /* u32 overflow of a CIGAR length sum (paf.rs:632-647)        */
} rb_status;

/* Rust slice::binary_search duplicate policy, low bit of `bsearch_policy`.
 * RB_LIFT_EARLY_EXIT may be OR-ed in: stop walking a record once all its windows are resolved
 * (same results; the reference always walks every record, so benchmarks leave it off). */
enum { RB_BSEARCH_MODERN = 0 /* rustc >= 1.82 (and < 1.52) */, RB_BSEARCH_LEGACY = 1 /* 1.52 .. 1.81 */, RB_LIFT_EARLY_EXIT = 16,
       /* RB_LIFT_DESCRIPTORS: do not copy the clipped cigars.  A host that still holds each record's cigar (the
        * reference does) only needs to know WHICH ops a clip keeps: for a row with RB_HIT_DESCRIPTOR set,
        * out_ops[out_off .. out_off + 4) = { first kept op (index into the record's ORIGINAL cigar), op count,
        * length of the first kept op, length of the last kept op }; every op in between is unchanged; a one-op clip
        * has length aln_len; RB_HIT_INSIDE rows keep all lengths.  Rows resolved by the generic kernel (irregular
        * cigars whose adjacent ops may merge) still carry real ops.  out_cap must be >= 4 * rows_cap + room for those. */
       RB_LIFT_DESCRIPTORS = 32,
       /* RB_LIFT_FUSED_SCAN (rb_dev_liftover, rb_dev_break): norm_rows is an OUTPUT.  rb_dev_scan_records need not have run: the call
        * looks at the ends of every record (remove_trailing_indels), verifies integrity and regularity while the clip kernel
        * streams the record, and runs the full record scan only for records that fail that check.  Rows of a record whose
        * norm row ends up with status != RB_ST_OK carry that status. */
       RB_LIFT_FUSED_SCAN = 64,
       /* RB_BREAK_ONE_WALK (rb_dev_break): the clip kernel finds the long indels itself while it streams a record (no separate pass
        * that collects the pieces first: the ops are read once).  The records this path does not take (irregular CIGARs, records
        * its verification hands back, boundaries only the generic kernel resolves) are declined one by one inside the same call:
        * their pieces are found in a pass of their own and the generic kernel clips them.  The results are complete either way. */
       RB_BREAK_ONE_WALK = 128,
       /* RB_LIFT_OP_STARTS (rb_dev_liftover, rb_dev_break; not with RB_LIFT_FUSED_SCAN or RB_LIFT_DESCRIPTORS): the batch is one that trim-paf has cut IN PLACE
        * (rb_dev_overlap_split with RB_TRIM_IN_PLACE + rb_dev_apply_pairs): batch->op_off[r] is where record r starts and says nothing
        * about where it ends, every extent comes from norm_rows (first_op, n_ops), which must be the finished rows of that batch.
        * The plan is the one built from the op offsets the batch had BEFORE the passes (records only shrink inside their old
        * extents, so its tiles still hold).  With it the README pipeline trim-paf | break-paf needs no rb_dev_gather_records
        * between the two: the clip kernels stream over the gaps the cuts left between the records of a tile.  A record a pass has
        * MOVED (an irregular record's clip, written behind the ops in use) lies at or behind batch->n_ops = the plan's op count: if the
        * passes moved any, gather first.  The call REFUSES otherwise: it checks every record whose norm row has status RB_ST_OK, and
        * returns RB_E_INVALID (rb_ctx_last_error names the record) before any clip kernel runs if [op_off[r] + first_op, + n_ops) is not
        * inside [0, batch->n_ops).  That check waits for the stream once.  Norm rows that are stale but whose extents stay inside the
        * batch are not caught: keeping them current is the caller's part. */
       RB_LIFT_OP_STARTS = 1 << 20,
       /* RB_LIFT_QBED (rb_host_liftover_text and rb_host_liftover_largest_text ONLY; rb_host_break_text returns RB_E_INVALID with it,
        * and no rb_dev_* entry point knows it -- the wrappers take the bit out of the policy before they call one): liftover --qbed, the
        * windows are in QUERY coordinates.  See rb_host_liftover_text below. */
       RB_LIFT_QBED = 1 << 21 };

/* rb_norm_row.flags / rb_reduce_row.flags */
enum {
    RB_F_REGULAR = 1u << 0,   /* only M I D N = X ops, every len >= 1, no two adjacent ops of one type, M / = / X at both ends */
    RB_F_STRIPPED = 1u << 1,  /* leading/trailing indels were removed (host appends _TO.<..>.<..>) */
    RB_F_HAS_M = 1u << 2,     /* cigar contains 'M' (bamstats.rs:145 warning)                      */
    RB_F_PROVISIONAL = 1u << 3, /* never visible to callers: row written from the record's ends only, not yet verified */
    RB_F_ENDS_NOT_MATCH = 1u << 4 /* never visible to callers: provisional row whose kept range does not start and end on M / = / X */
};
/* rb_hit_row.flags */
enum {
    RB_HIT_INSIDE = 1u << 0,  /* liftover.rs:23-25: record returned unchanged and keeps its OWN id */
    RB_HIT_GENERIC = 1u << 1, /* resolved by the generic (serial) kernel, informational             */
    RB_HIT_DESCRIPTOR = 1u << 2 /* out_ops holds a 4-word clip descriptor, not ops (RB_LIFT_DESCRIPTORS) */
};

/* ---- result rows (written by the device; 72 / 64 / 64 bytes) ---------------------------------- */
typedef struct rb_reduce_row { /* check_integrity + stats of the ORIGINAL record */
    uint64_t t_bases, q_bases;                  /* infer_n_bases: reference / query consuming      */
    uint32_t nmatch, aln_len;                   /* M+=+X lengths (quirk 9.3.1), all lengths        */
    uint32_t equal, diff, ins, del, matches;    /* bamstats.rs:26-30 (diff = X + M, matches = M)   */
    uint32_t ins_events, del_events;
    float id_by_all, id_by_events, id_by_matches; /* bamstats.rs:138-142, f32                      */
    uint32_t status;                            /* RB_ST_OK / PANIC_INTEGRITY_* / PANIC_OVERFLOW    */
    uint32_t flags;
} rb_reduce_row;

typedef struct rb_norm_row { /* the record after remove_trailing_indels (paf.rs:656-783) */
    uint64_t t_st, t_en, q_st, q_en;
    uint32_t first_op, n_ops;    /* kept op range, relative to the record's first op */
    uint32_t lead_ops, trail_ops;
    uint32_t nmatch, aln_len;    /* of the kept range */
    uint32_t status;
    uint32_t flags;
} rb_norm_row;

typedef struct rb_hit_row { /* one (record, window) pair that passed paf_overlaps_rgn */
    uint32_t rec, win;           /* record index in the batch; window index in BED order (break: piece #) */
    uint16_t status, flags;
    uint32_t out_n;              /* ops in the clipped cigar */
    uint64_t t_st, t_en, q_st, q_en;
    uint32_t nmatch, aln_len;
    uint64_t out_off;            /* first op of the clipped cigar in out_ops[] */
} rb_hit_row;

typedef struct rb_pair_row { /* trim-paf: one (left, right) overlap pair, 128 bytes */
    uint64_t split_idx;          /* trim_overlap.rs:69-76 */
    int32_t split_score;
    uint32_t status;
    uint64_t t_st[2], t_en[2], q_st[2], q_en[2]; /* [0]=left [1]=right after truncate_record_by_query */
    uint32_t nmatch[2], aln_len[2];
    uint64_t out_off[2];
    uint32_t out_n[2];
    uint64_t _pad;
} rb_pair_row;

typedef struct rb_counters { /* device-written job summary, 64 bytes */
    uint64_t n_hits;             /* rows the job wants to write: EXACT also when the call overflowed (it is the total of the hit scan,
                                    which does not depend on rows_cap or out_cap) -- except with brk_scratch_short, see there */
    uint64_t out_ops_needed;     /* upper bound of out_ops[] capacity that makes the job fit      */
    uint64_t out_ops_used;       /* highest op index written + 1                                  */
    uint64_t n_generic;          /* hits routed to the generic kernel                             */
    uint32_t overflow;           /* != 0: rows or out_ops capacity exceeded, results incomplete   */
    uint32_t phase[5];           /* diagnostics (debug_skip & 32): shader-clock sums per phase of the clip kernel, units of 16 cycles;
                                    without debug_skip: phase[3] = tiles of short records the call ran (0: none), phase[4] = records of
                                    those tiles that the tile kernel handed back to the per-record kernel (informational) */
    uint32_t brk_scratch_short;  /* RB_BREAK_ONE_WALK only: != 0: a scratch-row cursor ran out before the rows did (the scratch rows are shared out
                                    evenly among up to 256 cursors, the records are not); overflow is set, and n_hits is then NOT the row count but a
                                    rows_cap to try next -- above both the true count and the rows_cap of this call, a quarter and 1024 more each time.
                                    A caller that follows it gets there in a few calls (rb_host_break allows itself six) */
    uint32_t redo_two_walk;      /* always 0: kept for the layout (RB_BREAK_ONE_WALK declines records one by one inside the call) */
} rb_counters;

/* per-record outcome of rb_dev_parse_cigars */
enum { RB_TEXT_OK = 0, RB_TEXT_BAD = 1 /* the reference's "Unable to parse cigar string." panic */, RB_TEXT_TOO_LONG = 2 /* a length >= 2^28 */,
       RB_TEXT_UNUSUAL = 3 /* a number written with ten or more digits (zero padded, or past u32): not decided on the device, parse it on the host */ };

/* ---- views over caller-owned device memory ---------------------------------------------------- */
typedef struct rb_batch_view {
    uint64_t n_rec, n_ops;
    const uint32_t *ops;
    const uint64_t *op_off;
    const uint64_t *t_st, *t_en, *q_st, *q_en;
    const uint8_t *strand;
    const uint32_t *contig;
} rb_batch_view;

typedef struct rb_windows_view {
    uint64_t n_win;
    const uint32_t *contig;
    const uint64_t *st, *en;
} rb_windows_view;

typedef struct rb_ctx rb_ctx;
typedef struct rb_plan rb_plan; /* host-built schedule for one (batch, windows) pair */

/* ---- context ---------------------------------------------------------------------------------- */
int rb_abi_version(void);
int rb_device_count(void);
/* `hip_stream`: a hipStream_t to enqueue on (e.g. torch's current stream), or NULL for a private one. */
int rb_ctx_create(int device, void *hip_stream, rb_ctx **out);
void rb_ctx_destroy(rb_ctx *ctx);
const char *rb_ctx_last_error(const rb_ctx *ctx);
int rb_ctx_sync(rb_ctx *ctx);
void *rb_ctx_stream(rb_ctx *ctx);
/* Measurement aid: when enabled, every rb_dev_liftover / rb_dev_break call brackets its dominant
 * (streaming clip) kernel with HIP events on the context's stream.  rb_ctx_get_timing synchronises
 * and returns the per-call durations in milliseconds, oldest first (ring of the last 256 calls). */
int rb_ctx_set_timing(rb_ctx *ctx, int enabled);
int rb_ctx_get_timing(rb_ctx *ctx, double *ms_out, int cap, int *n_out);

/* Device memory.  Hosts that keep a batch resident across calls should take the batch, workspace, rows and
 * output arenas from here: requests of 256 MB and more are built from 2 MB physical chunks (hipMemCreate)
 * mapped into one virtual range, which spreads a multi-GB array evenly over the HBM channels whatever the
 * driver's free list looks like.  On the headline batch the clip kernel takes 9.3-9.4 ms per launch on such
 * memory against 10.2-11.9 ms on plain hipMalloc memory and 18-20 ms on one physically contiguous block
 * (profiles/r03_alloc_summary.md).  Smaller requests are plain hipMalloc.  RB_ALLOC_MODE in the environment
 * overrides: default (hipMalloc always) | chunks | scatter (chunks in shuffled order) | contiguous.
 * Pointers are 2 MB aligned when chunked, 256 B otherwise; free only with rb_dev_free. */
int rb_dev_alloc(rb_ctx *ctx, size_t bytes, void **dev_ptr);
int rb_dev_free(rb_ctx *ctx, void *dev_ptr);
/* which route a buffer of rb_dev_alloc took: 1 = 2 MB physical chunks, 0 = plain hipMalloc (a small request, or the fallback when the
 * chunked route failed -- the two routes differ by 10-20 % in the clip kernel's time, so bench.py reports it) */
int rb_dev_alloc_mode(rb_ctx *ctx, const void *dev_ptr);
/* ADDRESS SPACE.  A chunked buffer that is FREED gives its memory back, not its virtual range: on this ROCm a kernel's stores into a range
 * the process had mapped before went to the OLD physical pages (tools/alloc_probe2.py), so rb_dev_free retires the range for the life of
 * the process.  A host that allocates and frees 40-75 GB batches therefore spends that much address space per batch; the library counts it
 * and stops using the chunked route (plain hipMalloc instead: slower pages, rb_dev_alloc_mode says 0) once live + retired ranges reach
 * RB_ALLOC_VA_CAP_GB (default 32768 = 32 TB of the 128 TB a process has).  The way around it is not to free:
 *   rb_dev_release     gives a buffer back to the CONTEXT: it stays mapped, keeps its physical pages (and so what rb_dev_alloc_placed
 *                      chose them for), and the next rb_dev_alloc / rb_dev_alloc_placed[_by] of exactly the same size on this context
 *                      returns it -- no address space retired, no 14 us per chunk, no placement measured again (a released PLACED
 *                      buffer satisfies rb_dev_alloc_placed[_by] at once: *kept = -1, no score).  Buffers below 1 MB are simply freed.
 *                      The context's stream is synchronised; work on other streams must be finished.  At most RB_ALLOC_CACHE_GB
 *                      (default 96) gigabytes are held, the oldest are freed first; rb_ctx_destroy frees what is held.
 *   rb_dev_cache_trim  frees held buffers, oldest first, until at most keep_bytes remain.
 *   rb_dev_alloc_stats out[0] live chunked bytes (process), out[1] bytes this context holds for reuse, out[2] retired address space
 *                      (process), out[3] the cap on out[0] + out[2], out[4] requests of this context that fell back to plain hipMalloc. */
int rb_dev_release(rb_ctx *ctx, void *dev_ptr);
int rb_dev_cache_trim(rb_ctx *ctx, uint64_t keep_bytes);
int rb_dev_alloc_stats(rb_ctx *ctx, uint64_t out[5]);
/* Transfers of 8 MB and more go through the context's pinned staging ring (two page-locked 32 MB chunks, hipHostMalloc): the
 * host side of a chunk is copied on several host threads while the DMA of the other chunk runs, so pageable caller memory moves
 * at the link's rate and host_src may be reused as soon as rb_dev_upload returns (the DMAs are queued on the context's stream).
 * Smaller uploads are plain asynchronous copies: host_src must then stay valid until the stream has been synchronised. */
int rb_dev_upload(rb_ctx *ctx, void *dev_dst, const void *host_src, size_t bytes);   /* async with respect to the device */
int rb_dev_download(rb_ctx *ctx, void *host_dst, const void *dev_src, size_t bytes); /* synchronises */
int rb_dev_memset(rb_ctx *ctx, void *dev_dst, int value, size_t bytes);              /* async */

/* ---- K1: one pass over every record's ops ----------------------------------------------------- *
 * reduce_rows and/or norm_rows may be NULL.  [n_rec] each. */
int rb_dev_scan_records(rb_ctx *ctx, const rb_batch_view *batch, rb_reduce_row *reduce_rows, rb_norm_row *norm_rows);
/* Which kernel scanned what (tests, diagnostics; read-only).  rb_dev_scan_records has two kernels: a batch of at least 64 records whose
 * mean is at most 1536 ops takes the ROW FORM (a row of 16 lanes per record, four records to a wavefront), which leaves its records of
 * fewer than 4 or more than 2048 ops on a list for the wave-per-record kernel; every other batch goes to the wave-per-record kernel
 * whole.  Same rows either way.  After a call on this context: out[0] = records the row form scanned itself, out[1] = records it
 * listed; both 0 when the last call did not take the row form (or none was made).  Synchronises the context's stream and reads eight
 * bytes back; rb_dev_scan_records itself does nothing for it but remember the batch's record count. */
int rb_ctx_scan_route(rb_ctx *ctx, uint64_t out[2]);

/* ---- schedule (host side, no device work besides small uploads) ------------------------------- *
 * Built from HOST copies of the small per-record / per-window arrays:
 *   - canonical output order: contigs by first appearance, then record order (liftover.rs:151-164)
 *   - longest-first launch order (load balance; does not affect results)
 *   - windows grouped by contig in BED order, with a per-contig "monotone" flag
 *   - (round 5) TILES of short records: runs of records that lie one behind the other in ops[], 8 .. 2048 ops each, at most 32 of them and
 *     4064 ops together.  rb_dev_liftover / rb_dev_break stream a tile with ONE wavefront (k_tile.hip) instead of one per record; longer
 *     records keep the per-record kernel, and a tile the tile kernel does not take (an irregular or stripped record, an integrity failure,
 *     more than 64 hits, ...) is handed to it record by record.  Same rows, same clips either way; counters.phase[3..4] tell how it went.
 *     RB_TILE=0 in the environment switches the tiles off, RB_SHORT_MAX=<ops> moves the line (both read here, per plan).
 *     rb_dev_liftover runs the tile kernel on the context's side stream, beside the per-record kernel, when the batch has records of both
 *     kinds; RB_TILE_BESIDE=0 (read per call) keeps the call on one stream.
 * `windows` may be NULL (break-paf / stats only).  */
int rb_plan_create(rb_ctx *ctx, uint64_t n_rec, const uint64_t *op_off_host, const uint32_t *contig_host,
                   uint64_t n_win, const uint32_t *w_contig_host, const uint64_t *w_st_host, const uint64_t *w_en_host,
                   rb_plan **out);
void rb_plan_destroy(rb_plan *plan);
/* How rb_plan_create cuts a batch into tiles and orders its schedule, on plain host arrays (no device, no context): sched_out[n_rec] =
 * the records longer than short_max (0: the default, 2048) longest first -- *n_long_out of them --, then the others in memory order;
 * tiles_out[3 t ..] = {first record | pass-through << 31, records, schedule slot of the first record}.  Returns the number of tiles
 * (all of them are counted, tiles_cap of them written), -1 on bad arguments. */
int64_t rb_plan_tiles_host(uint64_t n_rec, const uint64_t *op_off_host, uint64_t short_max, uint32_t *sched_out, uint32_t *tiles_out,
                           uint64_t tiles_cap, uint64_t *n_long_out);
/* bytes of device workspace rb_dev_liftover / rb_dev_break need for this plan and row capacity (the workspace must be
 * 256-byte aligned, as rb_dev_alloc returns it) */
size_t rb_plan_workspace_bytes(const rb_plan *plan, uint64_t rows_cap);
/* diagnostics (bench.py's box block): byte offset, inside that workspace, of [n_rec] u32 words in which the diagnostics build of the
 * clip kernel leaves the 100 MHz clock (low 32 bits) at which the wave of schedule slot w was done.  Written only by calls whose
 * policy carries the undocumented debug bits; the product's kernels never touch the area. */
size_t rb_plan_diag_stamps_offset(const rb_plan *plan, uint64_t rows_cap);
/* out_ops capacity (in ops) with which rb_dev_liftover (for_break = 0) / rb_dev_break (1) can emit every clip while the record
 * streams past: the clipped cigars go to up to 4 positional copies of the batch's op index space (as many as the sorted window
 * lists overlap deep; two for break-paf), and only rows' out_off says where a clip is.  A smaller out_cap still works -- clips
 * without a place are then copied by a second kernel into what room there is, and counters report overflow / out_ops_needed as
 * before -- a larger one is never needed for sorted, at most 4-deep window lists. */
uint64_t rb_plan_out_capacity(const rb_plan *plan, int for_break);

/* ---- liftover --------------------------------------------------------------------------------- *
 * For every record (status OK in norm_rows) and every window of the same contig with
 * t_en > st && t_st < en, in canonical order, writes one rb_hit_row and the clipped cigar.
 *   rows      [rows_cap]      out_ops [out_cap]      counters [1]      workspace [rb_plan_workspace_bytes]
 * On capacity overflow counters->overflow != 0 and counters say what is needed; the caller
 * enlarges and calls again (the host wrapper below does that).  In full (tests/test_gpu_capacity.py):
 *   - the call returns RB_OK all the same, and writes nothing at or behind rows[rows_cap], out_ops[out_cap] and the end of the workspace:
 *     no slack is needed behind any of the three (rows_cap >= 1; the workspace is sized for the rows_cap of the call);
 *   - the rows and clips an overflowed call did write are incomplete and not specified;
 *   - n_hits is the exact number of rows, and a call with rows_cap = max(rows_cap, n_hits) and out_cap = max(out_cap, out_ops_needed),
 *     nothing added, does not overflow -- one-walk break-paf apart, which may ask again (rb_counters.brk_scratch_short);
 *   - out_ops_needed is an upper bound, not the least capacity that works (a call may fit into less): the slots the window lists ask
 *     for, and every arena behind them as large as the fullest one got, plus 1024 ops each -- clips without a slot are dealt to the
 *     arenas in the order they turn up, which may differ a little from call to call, and that room takes it up;
 *   - RB_LIFT_DESCRIPTORS: an out_cap below 4 * rows_cap + 1024 is refused with RB_E_CAPACITY before anything is written or enqueued. */
int rb_dev_liftover(rb_ctx *ctx, const rb_plan *plan, const rb_batch_view *batch, const rb_norm_row *norm_rows,
                    int bsearch_policy, void *workspace, rb_hit_row *rows, uint64_t rows_cap, uint32_t *out_ops,
                    uint64_t out_cap, rb_counters *counters);

/* ---- liftover --largest (main.rs:200-208) ------------------------------------------------------ *
 * The reference sorts the records of trim_paf_by_rgns stably by id and keeps, per id, the LAST record of largest t_en - t_st.  Here the
 * hit rows of rb_dev_liftover are reduced to one row per KEY where they lie: the host interns the id strings into dense u32 keys (in
 * ascending bytewise order of the strings, if sel[] is to come out in the reference's print order); the device never sees a string.
 *   key of row k   rec_key[rows[k].rec] if rows[k].flags & RB_HIT_INSIDE (liftover.rs:23-25: the record keeps its OWN id), else
 *                  win_key[rows[k].win] (liftover.rs:20).  Rows whose status is not RB_ST_OK take no part (the reference dropped them or
 *                  panicked) and their keys are not looked at; a row whose key is >= n_keys takes no part either and is counted in out[1].
 *   winner of a key the row of largest t_en - t_st (a full u64), among equals the LARGEST ROW INDEX: hit rows are in the order of the
 *                  reference's record list, so that is max_by_key's last maximum behind the stable sort.
 *   rows [n_rows] as rb_dev_liftover wrote them (16-byte aligned); win_key [n_win]; rec_key [n_rec] (NULL allowed only if no row is INSIDE: an
 *   INSIDE row then counts as a bad key); sel [n_keys] OUT: the winners' row indices, dense, in ascending key order; out: DEVICE memory,
 *   16 bytes OUT: out[0] = n_sel, out[1] = rows ignored because their key was >= n_keys (or rec_key was NULL); scratch:
 *   rb_largest_scratch_bytes(n_keys) bytes, 256-byte aligned, zeroed by the call itself on the stream, every time.  Enqueues on the context's
 *   stream, does not synchronise.  n_rows == 0 or n_keys == 0 is valid (n_sel = 0).  Two calls on the same rows write the same bytes. */
size_t rb_largest_scratch_bytes(uint64_t n_keys);
int rb_dev_largest(rb_ctx *ctx, const rb_hit_row *rows, uint64_t n_rows, const uint32_t *win_key, const uint32_t *rec_key,
                   uint64_t n_keys, uint64_t *sel, uint64_t *out, void *scratch);

/* ---- stats of the hit rows (`rb liftover .. | rb stats --paf` without the text in between) ------- *
 * <- bamstats::stats_from_paf (bamstats.rs:91-105, add_stats_from_cigar :107-154) + check_integrity (paf.rs:825-857) of every record
 *    that rb_dev_liftover / rb_dev_break produced, where its clip lies.
 * For a row k with status RB_ST_OK, stats[k] is what rb_dev_scan_records would write as the reduce row of a record that has the clip's
 * ops as its CIGAR and rows[k].t_st / t_en / q_st / q_en as its coordinates: t_bases, q_bases, nmatch, aln_len, the seven u32 counters
 * (diff = X + M, matches = M), the three f32 ratios (100.0f * (float)equal, divided by the u32 sum cast to float: NaN for a clip without
 * = X M I D, which no clip kernel writes: a clip starts on a match op), status = RB_ST_OK, or RB_ST_PANIC_INTEGRITY_T / _Q when the sums
 * disagree with the row's spans (RB_ST_PANIC_OVERFLOW when all lengths together pass 2^32 - 1) -- what Paf::from_file of the second
 * command would panic on; rows the clip kernels wrote never have it, so it is a self-check --, flags = RB_F_HAS_M or 0.
 * For a row whose status is not RB_ST_OK, stats[k] is all zero except status = rows[k].status.
 * Where the clip is:  without RB_HIT_DESCRIPTOR out_ops[out_off .. out_off + out_n).  With it d = out_ops + out_off and the ops are
 *   batch->ops[batch->op_off[rec] + d[0] ..][d[1]]; for rows without RB_HIT_INSIDE the first length is replaced by d[2] and the last by
 *   d[3] (0 = keep), a one-op clip with both takes d[2] + d[3] - len (= aln_len); RB_HIT_INSIDE rows keep all lengths (d[2], d[3] are not
 *   looked at).  batch->op_off[rec] is used as a START only, never op_off[rec + 1]: a batch in RB_LIFT_OP_STARTS form works.  Both forms
 *   may occur in one call (in descriptor mode the generic kernel's rows carry real ops).  Of `batch` only ops and op_off are read.
 * Op codes: all nine, with the scan's classes; a continuation word adds payload << 28 to its owner's class and is no event; other codes
 *   above 8 count as rb_dev_scan_records counts them (in aln_len alone).  Sums are 64 bits wide: a single `=` of 3e9 bases is legal.
 * MEMORY: the call reads the rows, whole 16-byte granules that hold at least one word of a clip or of a descriptor, op_off[rec] of
 *   descriptor rows, and nothing else; out_ops and batch->ops must be 16-byte aligned and readable up to the next multiple of four words
 *   behind the last clip (the batch's "next multiple of 32 ops" rule covers batch->ops).  It writes stats[0 .. n_rows) and nothing else.
 * Enqueues on the context's stream, does not synchronise.  n_rows == 0 is valid.  Two calls on the same rows write the same bytes. */
int rb_dev_stats_rows(rb_ctx *ctx, const rb_batch_view *batch, const rb_hit_row *rows, uint64_t n_rows, const uint32_t *out_ops,
                      rb_reduce_row *stats /* [n_rows] OUT */);

/* ---- the hit rows of a clip call as a batch (`rb break-paf .. | rb liftover ..` without the text in between) ---- *
 * The second command's Paf::from_file over what the first one printed: every row of rb_dev_liftover / rb_dev_break with status RB_ST_OK
 * becomes one record ("piece") of a new dense batch, in row order (for rb_dev_break: record order then piece order, the order
 * `rb break-paf` prints).  Rows of any other status produce nothing (the reference's None); a row with a status >= 16 (a panic) sets
 * info->declined, the caller replays the file on the record route.
 *   piece p of row k:  new_ops[new_op_off[p] .. new_op_off[p + 1]) = the clip's ops, found as rb_dev_stats_rows finds them (plain ops at
 *       out_ops[out_off ..][out_n]; a descriptor d = out_ops + out_off means src->ops[src->op_off[rec] + d[0] ..][d[1]], for rows without
 *       RB_HIT_INSIDE the first length replaced by d[2] and the last by d[3] (0 = keep), a one-op clip with both takes d[2] + d[3] - len);
 *       both forms may occur in one call.  src->op_off[rec] is used as a START only: a batch in RB_LIFT_OP_STARTS form works.
 *       t_st / t_en / q_st / q_en [p] = the row's; strand / contig [p] = src's at rows[k].rec; parent[p] = rows[k].rec.
 *       new_op_off is the exclusive prefix of the pieces' op counts, new_op_off[n_pieces] = n_ops: an ordinary batch.
 *   LENGTHS OF 2^28 AND MORE: a clip's words are copied as words, so a clip that holds RB_OP_CONT words (plain ops the generic kernel
 *       wrote; the clip kernels write no descriptor over a record that has one) is HANDLED: owner and continuation arrive together.  A
 *       descriptor's replaced first / last length (d[2], d[3], or d[2] + d[3] - len) of 2^28 and more would need a continuation word the
 *       piece has no place for: that DECLINES (info->declined != 0; the word written holds the low 28 bits).
 *   info (device memory, 64 B, written by every call): n_pieces and n_ops are EXACT whatever the capacities; overflow != 0: pieces_cap or
 *       ops_cap was too small and the outputs are incomplete; declined as above.
 *   new_ops == NULL: sizes only -- info is written (overflow 0) and nothing else; the other outputs may be NULL, the capacities are ignored.
 *   CAPACITY (tests/test_gpu_rows_to_batch.py, as tests/test_gpu_capacity.py states it for the clip calls): nothing is written at or behind
 *       new_ops[ops_cap], the per-piece arrays [pieces_cap], new_op_off[pieces_cap + 1] or the end of the scratch; a short call returns
 *       RB_OK with overflow set, and a second call with exactly the reported counts fits.
 *   MEMORY: reads the rows, whole aligned 16-byte groups that hold at least one word of a clip, the 16 bytes of a descriptor, and op_off /
 *       strand / contig of the rows' records; rows, out_ops, src->ops and new_ops must be 16-byte aligned, out_ops and src->ops readable up
 *       to the next multiple of four words behind the last clip.  Writes new_ops[0 .. n_ops), the per-piece arrays [0 .. n_pieces),
 *       new_op_off[0 .. n_pieces], info and the scratch (rb_rows_to_batch_scratch_bytes(n_rows) bytes, 256-byte aligned), nothing else:
 *       the caller leaves the batch's usual readable slack behind new_ops if it hands the pieces to a clip call.
 *   Enqueues on the context's stream, does not synchronise.  n_rows == 0 is valid.  Two calls on the same input write the same bytes.
 * rb_rows_to_batch_shape: the kernel's thresholds, for tests (no device needed): out[0] = ops per step of a row of 16 lanes, out[1] = the
 *   longest clip a row takes (longer ones are walked by the whole wavefront), out[2] = ops per step of the wavefront. */
typedef struct rb_pieces_info {
    uint64_t n_pieces, n_ops;
    uint32_t overflow;
    uint32_t declined;
    uint64_t _reserved[5];
} rb_pieces_info; /* 64 B */
size_t rb_rows_to_batch_scratch_bytes(uint64_t n_rows);
void rb_rows_to_batch_shape(uint32_t out[3]);
int rb_dev_rows_to_batch(rb_ctx *ctx, const rb_batch_view *src, const rb_hit_row *rows, uint64_t n_rows, const uint32_t *out_ops,
                         uint64_t pieces_cap, uint64_t ops_cap, uint32_t *new_ops, uint64_t *new_op_off /* [pieces_cap + 1] */,
                         uint64_t *t_st, uint64_t *t_en, uint64_t *q_st, uint64_t *q_en, uint8_t *strand, uint32_t *contig,
                         uint32_t *parent /* each [pieces_cap] */, rb_pieces_info *info, void *scratch);

/* ---- orient / filter over hit rows (`rb break-paf .. | rb orient - | rb filter .. -` without the text in between) ---- *
 * <- Paf::orient (paf.rs:114-157, without the order column that only --scaffold reads) and main.rs:242-244: filter_query_len, filter_aln_len,
 *    filter_aln_pairs (paf.rs:91-111), over the records the second command's Paf::from_file reads: every row of a clip call with status
 *    RB_ST_OK, in row order.  Neither command touches a CIGAR; both are sums keyed by the record's (target name, query name) pair.  The host
 *    interns the pairs into dense u32 keys per RECORD (orient appends + or - to every query name of a pair alike, so the pairs in front of the
 *    filter are the same); the device never sees a string.
 *   takes part   a row with status RB_ST_OK, rec < n_rec and rec_key[rec] < n_keys.  Rows of another status count nowhere and produce
 *                nothing; an OK row without a valid key counts nowhere either and DECLINES.
 *   orient       (RB_PAIRS_ORIENT) per key, over the rows that take part: orient = sum of +(q_en - q_st) where strand[rec] is not '-' and
 *                -(q_en - q_st) where it is, as i64.  key_flip[key] = orient < 0 (strict: a sum of exactly 0 is not flipped); a flipped row
 *                gets q_st' = q_len - q_en, q_en' = q_len - q_st (mod 2^64) with q_len = rec_q_len[rec].  The host derives the name suffix
 *                and the printed strand from key_flip.  Without the bit key_flip is all zero.
 *   filter       (RB_PAIRS_FILTER) a row passes if rec_q_len[rec] > min_query and t_en - t_st > min_aln; fspan[key] = sum of t_en - t_st
 *                (u64) over the rows that PASS, and a row is kept if it passes and paired_len < fspan[key].  All three are strict.  Without
 *                the bit every row that takes part is kept.
 *   rows_out     [rows_cap] the kept rows, dense, in row order: 64-byte copies, q_st / q_en rewritten where the key is flipped, everything
 *                else -- out_off and flags too -- as it was, so rb_dev_stats_rows, rb_dev_format_cigars and rb_dev_rows_to_batch work on
 *                rows_out with the same batch and out_ops.
 *   info         (device memory, 64 B, written by every call) n_kept is EXACT whatever rows_cap; n_flipped_rows = kept rows of flipped keys;
 *                overflow != 0: rows_cap was too small, rows_out is incomplete; declined = the OR of RB_PAIRS_DECL_* -- the caller replays
 *                the file on the record route, the other outputs are still what the rules above say:
 *                  _PANIC      a row has a status >= 16 (the first command panicked part-way)
 *                  _KEY        a row with status RB_ST_OK has rec >= n_rec or rec_key[rec] >= n_keys
 *                  _WRAP       a row of a flipped key has q_len < q_en: the reference's subtraction wraps (or panics, by the build)
 *                  _ZERO_SPAN  (RB_PAIRS_ORIENT only) a key that has rows has a total t_en - t_st of 0: orient divides by it (paf.rs:143).
 *                              A piece of break-paf never has span 0: a self-check.
 *   CAPACITY (tests/test_gpu_pairs_rows.py): nothing is written at or behind rows_out[rows_cap], key_flip[n_keys] or the end of the scratch;
 *       a short rows_cap (0 too: rows_out may then be NULL) returns RB_OK with overflow set, and a second call with exactly n_kept fits.
 *   MEMORY: reads rows[0 .. n_rows) as whole 16-byte pieces (rows and rows_out must be 16-byte aligned), rec_key / rec_q_len / strand at the
 *       rows' records, nothing else.  Writes rows_out[0 .. min(n_kept, rows_cap)), key_flip[0 .. n_keys), info and the scratch
 *       (rb_pairs_scratch_bytes(n_keys, n_rows) bytes, 256-byte aligned; the sums in it are zeroed by the call itself on the stream, every time).
 *   Enqueues on the context's stream, does not synchronise.  n_rows == 0 and n_keys == 0 are valid; n_rows must be below 2^32 (RB_E_INVALID
 *   otherwise: 256 GB of rows).  Two calls on the same input write the same
 *   bytes: the sums are integers, the same in whatever order they are added, and the rows are placed by an exclusive scan, not by an atomic.
 * rb_pairs_shape: the sum kernel's shape, for tests (no device needed): out[0] = consecutive rows one wavefront sums (it carries an open run of
 *   one key from one group of 64 rows to the next), out[1] = rows per workgroup.
 * rb_host_pairs_rows: the same rules in plain C++ on HOST arrays, no device and no context (the record route's self-check and the tests' second
 *   opinion); same outputs, byte for byte.  Returns RB_OK or RB_E_INVALID. */
enum { RB_PAIRS_ORIENT = 1, RB_PAIRS_FILTER = 2 };
enum { RB_PAIRS_DECL_PANIC = 1, RB_PAIRS_DECL_KEY = 2, RB_PAIRS_DECL_WRAP = 4, RB_PAIRS_DECL_ZERO_SPAN = 8 };
typedef struct rb_pairs_info {
    uint64_t n_kept, n_flipped_rows;
    uint32_t overflow;
    uint32_t declined;
    uint64_t _reserved[5];
} rb_pairs_info; /* 64 B */
size_t rb_pairs_scratch_bytes(uint64_t n_keys, uint64_t n_rows);
void rb_pairs_shape(uint32_t out[2]);
int rb_dev_pairs_rows(rb_ctx *ctx, const rb_hit_row *rows, uint64_t n_rows, const uint32_t *rec_key, const uint64_t *rec_q_len,
                      const uint8_t *strand /* each [n_rec] */, uint64_t n_rec, uint64_t n_keys, uint32_t mode, uint64_t paired_len,
                      uint64_t min_aln, uint64_t min_query, rb_hit_row *rows_out, uint64_t rows_cap, uint8_t *key_flip /* [n_keys] OUT */,
                      rb_pairs_info *info, void *scratch);
int rb_host_pairs_rows(const rb_hit_row *rows, uint64_t n_rows, const uint32_t *rec_key, const uint64_t *rec_q_len, const uint8_t *strand,
                       uint64_t n_rec, uint64_t n_keys, uint32_t mode, uint64_t paired_len, uint64_t min_aln, uint64_t min_query,
                       rb_hit_row *rows_out, uint64_t rows_cap, uint8_t *key_flip, rb_pairs_info *info);

/* ---- orient [--scaffold] / filter over the RECORDS of a batch (`rb orient`, `rb filter` on a file's records) ---- *
 * <- Paf::orient (paf.rs:114-157) with the order column that --scaffold sorts by, and main.rs:242-244 (the three filters), over the records of
 *    a batch: the sums, the flags and the placement of rb_dev_pairs_rows, a record where that call has a hit row.  rec_key as there: the host's
 *    dense u32 key of each record's (target name, query name) pair.
 *   takes part   a record with rec_key[r] < n_keys.  A record with another key counts nowhere, is not kept, and DECLINES (_KEY).
 *   orient       (RB_PAIRS_ORIENT) per key, over the records that take part: orient = i64 sum of +(q_en - q_st) where strand[r] is not '-' and
 *                -(q_en - q_st) where it is; tspan = sum of w = t_en - t_st; order = sum of (w * (t_st + t_en)) / 2 -- product and sums mod
 *                2^64, as a release build of the reference.  key_flip[k] = orient < 0 (strict); key_order[k] = order / tspan where tspan != 0,
 *                else 0 (a record's `order`, paf.rs:143).  A key that has records and tspan == 0 is the reference's divide-by-zero panic: _ZERO_SPAN.
 *                q_st_out / q_en_out [n_rec]: q_len - q_en, q_len - q_st (mod 2^64) for the records of flipped keys, the input's for all others
 *                (a flipped record with q_len < q_en: _WRAP, the outputs are still the values mod 2^64).  Without the bit key_flip and
 *                key_order are all zero.
 *   filter       (RB_PAIRS_FILTER) a record passes if rec_q_len[r] > min_query and t_en - t_st > min_aln; fspan[key] = sum of t_en - t_st over
 *                the records that PASS; a record is kept if it passes and paired_len < fspan[key].  All three strict.  Without the bit every
 *                record that takes part is kept.  Orient's sums see every record that takes part, whatever the filter says.
 *   kept         [kept_cap] the indices of the kept records, ascending.
 *   info         as rb_dev_pairs_rows: n_kept and n_flipped_rows (kept records of flipped keys) EXACT whatever kept_cap; overflow != 0: kept_cap
 *                was too small (kept_cap == 0 with kept == NULL is allowed); declined = the OR of RB_PAIRS_DECL_KEY / _WRAP / _ZERO_SPAN.
 *   CAPACITY (tests/test_gpu_pairs_records.py): nothing is written at or behind kept[kept_cap], key_flip[n_keys], key_order[n_keys],
 *       q_*_out[n_rec] or the end of the scratch (rb_pairs_records_scratch_bytes(n_keys, n_rec) bytes, 256-byte aligned; the sums in it are
 *       zeroed by the call itself, every time); a second call with exactly n_kept fits.
 *   q_st_out / q_en_out may both be NULL, key_order may be NULL.  n_rec == 0 and n_keys == 0 are valid.  n_rec >= 2^32, an unknown mode bit or a
 *   misaligned pointer (u64 columns and info 8 bytes, u32 columns 4, the scratch 256): RB_E_INVALID before anything is enqueued.
 *   Enqueues on the context's stream, does not synchronise.  Two calls on the same input write the same bytes: integer sums, and nothing is
 *   placed or counted by an atomic.
 * rb_pairs_records_shape: out[0] = consecutive records one wavefront sums (it carries an open run of one key through them), out[1] = records
 *   per workgroup; no device needed.
 * rb_host_pairs_records: the same rules in plain C++ on HOST arrays, no context and no scratch; same outputs, byte for byte. */
size_t rb_pairs_records_scratch_bytes(uint64_t n_keys, uint64_t n_rec);
void rb_pairs_records_shape(uint32_t out[2]);
int rb_dev_pairs_records(rb_ctx *ctx, const uint64_t *t_st, const uint64_t *t_en, const uint64_t *q_st, const uint64_t *q_en,
                         const uint8_t *strand, const uint32_t *rec_key, const uint64_t *rec_q_len /* each [n_rec], device */,
                         uint64_t n_rec, uint64_t n_keys, uint32_t mode /* RB_PAIRS_ORIENT | RB_PAIRS_FILTER */,
                         uint64_t paired_len, uint64_t min_aln, uint64_t min_query,
                         uint32_t *kept /* [kept_cap] OUT */, uint64_t kept_cap, uint64_t *q_st_out, uint64_t *q_en_out /* [n_rec] OUT, may both be NULL */,
                         uint8_t *key_flip /* [n_keys] OUT */, uint64_t *key_order /* [n_keys] OUT, may be NULL */, rb_pairs_info *info, void *scratch);
int rb_host_pairs_records(const uint64_t *t_st, const uint64_t *t_en, const uint64_t *q_st, const uint64_t *q_en, const uint8_t *strand,
                          const uint32_t *rec_key, const uint64_t *rec_q_len, uint64_t n_rec, uint64_t n_keys, uint32_t mode, uint64_t paired_len,
                          uint64_t min_aln, uint64_t min_query, uint32_t *kept, uint64_t kept_cap, uint64_t *q_st_out, uint64_t *q_en_out,
                          uint8_t *key_flip, uint64_t *key_order, rb_pairs_info *info);

/* ---- break-paf -------------------------------------------------------------------------------- *
 * Pieces between indels longer than max_size, record order then piece order; same row shape,
 * rb_hit_row.win = piece ordinal among the candidate windows of the record. */
int rb_dev_break(rb_ctx *ctx, const rb_plan *plan, const rb_batch_view *batch, const rb_norm_row *norm_rows,
                 uint32_t max_size, int bsearch_policy, void *workspace, rb_hit_row *rows, uint64_t rows_cap,
                 uint32_t *out_ops, uint64_t out_cap, rb_counters *counters);

/* ---- invert ----------------------------------------------------------------------------------- *
 * out_ops[op_off[r] .. op_off[r+1]) = I<->D swapped, order reversed when strand[r] == '-' (an op and its RB_OP_CONT word
 * keep their order).  (The header swap t<->q is a host-side field swap.)  Where out_ops may lie:
 *   - fully outside [batch->ops, batch->ops + batch->n_ops): the batch is left as it is, the result goes to out_ops;
 *   - out_ops == batch->ops: IN PLACE, every record is swapped where it lies and the batch's original CIGARs are gone after the
 *     call (a batch the size of the device's memory needs no second array); calling it twice restores the batch;
 *   - inside that range but not equal to batch->ops: RB_E_INVALID (rb_ctx_last_error says so), no kernel runs. */
int rb_dev_swap(rb_ctx *ctx, const rb_batch_view *batch, uint32_t *out_ops);

/* ---- trim-paf: one pass of independent (left, right) overlap pairs ------------------------------ *
 * left[i] / right[i] index records of the batch (left = smaller q_st, paf.rs:252-256).  For each pair:
 * split point = first arg-max of prefix(left scores) + suffix(right scores) over the overlapped query
 * bases (trim_overlap.rs:50-76), then both records are clipped by query range.  pair_out_off[i] = first
 * op of pair i's output in out_ops; the pair needs room for n_ops(left) + n_ops(right) ops.  norm_rows
 * come from rb_dev_scan_records on the same batch.
 * RB_TRIM_IN_PLACE OR-ed into bsearch_policy (out_ops must then be batch->ops, the resident-batch set-up of rb_dev_apply_pairs):
 * a clip by query range keeps a RUN of the record's ops and changes only the lengths of the run's first and last op, so a pair of
 * regular records is not copied -- the two end words are rewritten where they are and rows[].out_off points at the run inside the
 * array (out_n = its length).  The record's ops outside the run stay where they were, no longer part of it; the batch's original
 * CIGARs are gone after the call.  Pairs with an irregular record still write their clips at pair_out_off. */
enum { RB_TRIM_IN_PLACE = 256 };
int rb_dev_overlap_split(rb_ctx *ctx, const rb_batch_view *batch, const rb_norm_row *norm_rows, uint64_t n_pairs,
                         const uint32_t *left, const uint32_t *right, const uint64_t *pair_out_off, int match_score,
                         int diff_score, int indel_score, int bsearch_policy, rb_pair_row *rows, uint32_t *out_ops);

/* rb_dev_trim_reserve (optional): rb_dev_overlap_split keeps, per context, a list of the pairs its first kernel leaves to the ones
 * behind it; the list grows with the largest n_pairs seen, and growing means a stream synchronisation and an allocation inside that
 * call.  A host that knows how many pairs a pass can have (one per query group) sizes the list up front with this.
 * The list (4 bytes per pair) is mandatory: if it cannot be allocated, this call and rb_dev_overlap_split return RB_E_NOMEM
 * (rb_ctx_last_error says so) and no kernel runs -- there is no slower route without it. */
int rb_dev_trim_reserve(rb_ctx *ctx, uint64_t n_pairs);

/* ---- trim-paf with the batch resident on the device across the passes of Paf::overlapping_paf_recs (paf.rs:210-305) ----------
 * rb_dev_apply_pairs: the records a pass has cut become the batch's current records.  For every pair k with status RB_ST_OK and
 *     side s (0 = left[k], 1 = right[k]):  op_off[rec] = rows[k].out_off[s] and norm_rows[rec] = the clipped record (coordinates,
 *     nmatch, aln_len, first_op 0, n_ops = out_n; a clip starts and ends on a match op, so the remove_trailing_indels of the next
 *     pass, paf.rs:218-220, finds nothing to strip).  out_off must index the SAME array as the batch's ops: call
 *     rb_dev_overlap_split with out_ops = batch->ops and pair_out_off pointing behind the ops in use.  From then on op_off is a
 *     table of starts, no longer a prefix array: only rb_dev_overlap_split, rb_dev_gather_records and rb_dev_format_cigars -- which
 *     take a record's extent from norm_rows / explicit counts -- may be used on the batch.
 * rb_dev_gather_records: the current records (ops[op_off[r] + first_op ..][n_ops], records whose status is not RB_ST_OK count as
 *     empty) copied into a dense array in record order; new_op_off [n_rec + 1] is its exclusive prefix.  new_ops NULL: sizes only.
 *     scratch: rb_text_scratch_bytes(n_rec) bytes.  The dense array with the coordinates of norm_rows is an ordinary batch again
 *     (e.g. for rb_dev_break: the README pipeline trim-paf | break-paf). */
int rb_dev_apply_pairs(rb_ctx *ctx, uint64_t n_pairs, const uint32_t *left, const uint32_t *right, const rb_pair_row *rows,
                       uint64_t *op_off, rb_norm_row *norm_rows);

/* rb_dev_trim_select: which pairs a pass of Paf::overlapping_paf_recs cuts, found on the device (paf.rs:223-284: the pair scan per
 *     query name over bed::get_overlap, the contained flags :244-249, "pairs by overlap descending, then the first pair of every
 *     query name" :262-284 = per group the pair of largest overlap, among equals the first in scan order).  order [n_rec] = the
 *     records stably sorted by query name (:223), grp_off [n_groups + 1] = where the groups of equal names begin in it (both device
 *     arrays the caller builds once).  Outputs: contained [n_rec] by RECORD (this pass's flags: the ones that count are the last
 *     pass's, :224), the chosen pairs dense in left / right / pair_out_off (room for n_groups each; pair k writes its clips at
 *     pair_out_off[k] >= out_base, n_ops(left) + n_ops(right) apart), and *pass (device memory, 64 bytes): n_pairs, n_deferred (pairs
 *     left for a later pass: the recursion of :286-288 goes on while it is not 0; the exact count as long as no single query group
 *     leaves more than (2^32 - 1) / n_groups pairs, a lower bound above that), ops_end (first op behind this pass's clips).
 *     scratch: rb_trim_select_scratch_bytes(n_groups).  Then rb_dev_overlap_split + rb_dev_apply_pairs on the n_pairs pairs, and
 *     rb_dev_trim_check folds the pair rows' statuses into pass->bad_status (0: every pair was cut). */
typedef struct rb_trim_pass {
    uint64_t n_pairs, n_deferred, ops_end;
    uint32_t bad_status, _pad;
    uint64_t _reserved[4];
} rb_trim_pass; /* 64 B */
size_t rb_trim_select_scratch_bytes(uint64_t n_groups);
int rb_dev_trim_select(rb_ctx *ctx, uint64_t n_rec, uint64_t n_groups, const uint32_t *order, const uint64_t *grp_off,
                       const rb_norm_row *norm_rows, uint64_t out_base, uint8_t *contained, uint32_t *left, uint32_t *right,
                       uint64_t *pair_out_off, rb_trim_pass *pass, void *scratch);
int rb_dev_trim_check(rb_ctx *ctx, uint64_t n_pairs, const rb_pair_row *rows, rb_trim_pass *pass);
int rb_dev_gather_records(rb_ctx *ctx, uint64_t n_rec, const uint32_t *ops, const uint64_t *op_off, const rb_norm_row *norm_rows,
                          uint64_t *new_op_off, uint32_t *new_ops, void *scratch);

/* ---- host-buffer wrappers (H2D, kernels, D2H; results malloc'ed, free with rb_host_free) ------ */
int rb_host_scan_records(rb_ctx *ctx, uint64_t n_rec, const uint32_t *ops, const uint64_t *op_off,
                         const uint64_t *t_st, const uint64_t *t_en, const uint64_t *q_st, const uint64_t *q_en,
                         const uint8_t *strand, rb_reduce_row *reduce_rows, rb_norm_row *norm_rows);
int rb_host_liftover(rb_ctx *ctx, uint64_t n_rec, const uint32_t *ops, const uint64_t *op_off, const uint64_t *t_st,
                     const uint64_t *t_en, const uint64_t *q_st, const uint64_t *q_en, const uint8_t *strand,
                     const uint32_t *contig, uint64_t n_win, const uint32_t *w_contig, const uint64_t *w_st,
                     const uint64_t *w_en, int bsearch_policy, rb_norm_row *norm_rows_out /* [n_rec] or NULL */,
                     rb_hit_row **rows, uint64_t *n_rows, uint32_t **out_ops, uint64_t *n_out, rb_counters *counters);
int rb_host_break(rb_ctx *ctx, uint64_t n_rec, const uint32_t *ops, const uint64_t *op_off, const uint64_t *t_st,
                  const uint64_t *t_en, const uint64_t *q_st, const uint64_t *q_en, const uint8_t *strand,
                  uint32_t max_size, int bsearch_policy, rb_norm_row *norm_rows_out, rb_hit_row **rows,
                  uint64_t *n_rows, uint32_t **out_ops, uint64_t *n_out, rb_counters *counters);
int rb_host_swap(rb_ctx *ctx, uint64_t n_rec, const uint32_t *ops, const uint64_t *op_off, const uint8_t *strand,
                 uint32_t *out_ops);
/* rows [n_pairs] caller-allocated; out_ops malloc'ed (dense, rows' out_off rebased onto it) */
int rb_host_overlap_split(rb_ctx *ctx, uint64_t n_rec, const uint32_t *ops, const uint64_t *op_off, const uint64_t *t_st,
                          const uint64_t *t_en, const uint64_t *q_st, const uint64_t *q_en, const uint8_t *strand,
                          uint64_t n_pairs, const uint32_t *left, const uint32_t *right, int match_score, int diff_score,
                          int indel_score, int bsearch_policy, rb_pair_row *rows, uint32_t **out_ops, uint64_t *n_out);
void rb_host_free(void *p);

/* ---- CIGAR text <-> packed ops on the device (the data format either side of the path) ----------
 *
 * rb_dev_parse_cigars   <- CigarString::try_from(value.as_bytes()).expect(..)       paf.rs:398-399
 *     text      device bytes holding the CIGAR strings of n_rec records (the `cg:Z:` values, without the tag);
 *               16-byte aligned, readable up to the next multiple of 16 past the last string
 *     text_off  [n_rec + 1] start of every string;  text_end [n_rec] or NULL (NULL: strings are back to back)
 *     op_off    [n_rec + 1] OUT  exclusive prefix of ops per record (op_off[n_rec] = total)
 *     ops       OUT, capacity ops_cap (total text bytes / 2 is always enough: an op is at least two characters)
 *     status    [n_rec] OUT  RB_TEXT_OK / RB_TEXT_BAD (the reference panics: "Unable to parse cigar string.") /
 *               RB_TEXT_TOO_LONG (a length >= 2^28 cannot be packed; the reference would go on)
 *     scratch   rb_text_scratch_bytes(n_rec) bytes
 *     TRUNCATION: the call returns RB_OK whatever ops_cap is, and op_off and status are exact whatever it is: the caller detects a
 *               short ops[] by op_off[n_rec] > ops_cap.  Nothing is written at or behind ops[ops_cap]; ops[0 .. ops_cap) are then the
 *               first ops_cap ops of the full result.
 * rb_dev_format_cigars  <- impl Display for CigarString inside impl Display for PafRecord   paf.rs:923-944
 *     item i prints ops[first[i] .. first[i] + count[i]) as <len><op>...; first_len / last_len (arrays or NULL,
 *     0 = keep) replace the length of the first / last op -- the clip descriptors of RB_LIFT_DESCRIPTORS:
 *     {first kept op, op count, first length, last length}; a one-op item with both prints first + last - len.
 *     ops_alt   optional second source array: an item whose first[] has bit 63 set takes its ops from ops_alt[]
 *               (clips the generic kernel copied out live in out_ops[], descriptor clips point into the batch)
 *     text_off  [n_items + 1] OUT exclusive prefix of bytes;  text OUT (NULL: sizes only; 16-byte aligned), capacity text_cap
 *               (11 bytes per op suffice)
 *     TRUNCATION: the call returns RB_OK whatever text_cap is, and text_off is exact whatever it is: the caller detects a short text[]
 *               by text_off[n_items] > text_cap.  Nothing is written at or behind text[text_cap].  Below it every item that ends at or
 *               in front of the last 16-byte boundary <= text_cap is printed whole; of the other items any byte may be missing (text is
 *               stored in steps of up to 255 ops, and a step that would end behind text_cap is left out whole), and a byte that is
 *               there is the right one.  Nothing else about the content is specified (tests/test_gpu_capacity.py).
 * rb_host_liftover_text: liftover from CIGAR text to CIGAR text.  text holds the records' `cg:Z:` values at
 *     [cig_off[r], cig_end[r]); they are parsed on the device (cig_status[r] = RB_TEXT_*; if any is not OK nothing else
 *     is computed), scanned (reduce_out / norm_out, either may be NULL), lifted over the windows in descriptor mode, and the
 *     clipped CIGAR of every hit row is printed on the device: row k's text is row_text[row_text_off[k] .. [k + 1]) (empty
 *     for rows whose status is not RB_ST_OK).  rows / row_text_off / row_text are malloc'ed (rb_host_free).
 *     With RB_LIFT_QBED in bsearch_policy (liftover --qbed, liftover.rs:139-148 in front of the same route): the caller passes the records
 *     as read from the file -- t_st, t_en, q_st, q_en, strand unswapped, cig_off / cig_end as above -- and only contig is different: it
 *     is the caller's interning of the records' QUERY names, the names w_contig refers to.  Then, in this order: the CIGARs are parsed;
 *     the records AS READ are scanned for reduce_out (Paf::from_file's check_integrity, paf.rs:70, is the original record's: a record
 *     whose target span disagrees with its CIGAR reports RB_ST_PANIC_INTEGRITY_T -- also when its query span disagrees too -- where a
 *     scan of the swapped record would report _Q for a target span that alone is off, and the I / D counters would change places); rb_dev_swap swaps the parsed ops in place (paf.rs:1050-1065); the batch with its t and q columns exchanged is scanned
 *     again for norm_out (the swapped record's remove_trailing_indels: first_op, lead_ops, trail_ops count ops of the SWAPPED CIGAR);
 *     liftover, --largest and the printing run as without the flag on that batch.  Hit rows are in the swapped frame: t_st / t_en are
 *     positions on the file's query sequence, q_st / q_en on its target, and the row text is a clip of the swapped CIGAR.
 * rb_host_liftover_largest_text: the same for liftover --largest.  win_key [n_win] and inside_key (the key of the empty id "", which a record
 *     read from a file has) are keys below n_keys (n_keys < 2^32 - 1).  The hit rows stay on the device; rb_dev_largest picks one per key,
 *     and only those rows are downloaded, given format items and printed: rows / row_text_off / row_text come back with n_sel entries in
 *     ascending key order, rows[].rec and rows[].win still index the input.  *declined != 0: nothing was selected and *n_rows = 0, the
 *     caller takes the record route --  1: a record whose norm row has RB_F_STRIPPED has an OK INSIDE row (its id carries a _TO.<lead>.<trail>
 *     suffix, paf.rs:726-731, that no key stands for; minimap2-style input has no such record); 2: some hit row has a status of
 *     RB_ST_PANIC_NOTFOUND or above (the reference panics inside trim_paf_by_rgns, before it selects).
 */
size_t rb_text_scratch_bytes(uint64_t n);
int rb_dev_parse_cigars(rb_ctx *ctx, const uint8_t *text, const uint64_t *text_off, const uint64_t *text_end, uint64_t n_rec,
                        uint64_t *op_off, uint32_t *ops, uint64_t ops_cap, uint8_t *status, void *scratch);
int rb_dev_format_cigars(rb_ctx *ctx, const uint32_t *ops, const uint32_t *ops_alt, uint64_t n_items, const uint64_t *first,
                         const uint32_t *count, const uint32_t *first_len, const uint32_t *last_len, uint64_t *text_off, uint8_t *text,
                         uint64_t text_cap, void *scratch);
/* host-buffer forms: H2D, kernels, D2H.  *ops / *text are malloc'ed (rb_host_free) */
int rb_host_parse_cigars(rb_ctx *ctx, const uint8_t *text, const uint64_t *text_off, const uint64_t *text_end, uint64_t n_rec,
                         uint64_t *op_off, uint32_t **ops, uint8_t *status);
int rb_host_format_cigars(rb_ctx *ctx, const uint32_t *ops, uint64_t n_ops, uint64_t n_items, const uint64_t *first, const uint32_t *count,
                          const uint32_t *first_len, const uint32_t *last_len, uint64_t *text_off, uint8_t **text);
int rb_host_liftover_text(rb_ctx *ctx, uint64_t n_rec, const uint8_t *text, uint64_t text_bytes, const uint64_t *cig_off,
                          const uint64_t *cig_end, const uint64_t *t_st, const uint64_t *t_en, const uint64_t *q_st, const uint64_t *q_en,
                          const uint8_t *strand, const uint32_t *contig, uint64_t n_win, const uint32_t *w_contig, const uint64_t *w_st,
                          const uint64_t *w_en, int bsearch_policy, uint8_t *cig_status, rb_reduce_row *reduce_out, rb_norm_row *norm_out,
                          rb_hit_row **rows, uint64_t *n_rows, uint64_t **row_text_off, uint8_t **row_text, rb_counters *counters);
int rb_host_liftover_largest_text(rb_ctx *ctx, uint64_t n_rec, const uint8_t *text, uint64_t text_bytes, const uint64_t *cig_off,
                                  const uint64_t *cig_end, const uint64_t *t_st, const uint64_t *t_en, const uint64_t *q_st, const uint64_t *q_en,
                                  const uint8_t *strand, const uint32_t *contig, uint64_t n_win, const uint32_t *w_contig, const uint64_t *w_st,
                                  const uint64_t *w_en, int bsearch_policy, uint8_t *cig_status, rb_reduce_row *reduce_out, rb_norm_row *norm_out,
                                  rb_hit_row **rows, uint64_t *n_rows, uint64_t **row_text_off, uint8_t **row_text, rb_counters *counters,
                                  const uint32_t *win_key, uint64_t n_keys, uint32_t inside_key, int *declined);
/* the same around rb_dev_break (break-paf, main.rs:271-281), and the record scan alone (stats --paf, main.rs:50-58) */
int rb_host_break_text(rb_ctx *ctx, uint64_t n_rec, const uint8_t *text, uint64_t text_bytes, const uint64_t *cig_off,
                       const uint64_t *cig_end, const uint64_t *t_st, const uint64_t *t_en, const uint64_t *q_st, const uint64_t *q_en,
                       const uint8_t *strand, uint32_t max_size, int bsearch_policy, uint8_t *cig_status, rb_reduce_row *reduce_out,
                       rb_norm_row *norm_out, rb_hit_row **rows, uint64_t *n_rows, uint64_t **row_text_off, uint8_t **row_text,
                       rb_counters *counters);
/* the same two without any text out (`rb liftover --stats`, `rb break-paf --stats`: what `.. | rb stats --paf` prints needs no CIGAR text):
 * parse, scan, clip in descriptor mode, rb_dev_stats_rows on the rows and clips where they lie, then rows and stats to the host.
 * rb_dev_format_cigars does not run.  Arguments as rb_host_liftover_text / rb_host_break_text up to n_rows; *stats [*n_rows] (malloc'ed,
 * rb_host_free) takes the place of row_text_off / row_text: the reduce row of row k's clip, as rb_dev_stats_rows defines it.
 * RB_LIFT_QBED works as in rb_host_liftover_text: rows, clips and therefore stats are in the swapped frame (I and D have changed places,
 * as they have in the text the plain command prints). */
int rb_host_liftover_stats_text(rb_ctx *ctx, uint64_t n_rec, const uint8_t *text, uint64_t text_bytes, const uint64_t *cig_off,
                                const uint64_t *cig_end, const uint64_t *t_st, const uint64_t *t_en, const uint64_t *q_st, const uint64_t *q_en,
                                const uint8_t *strand, const uint32_t *contig, uint64_t n_win, const uint32_t *w_contig, const uint64_t *w_st,
                                const uint64_t *w_en, int bsearch_policy, uint8_t *cig_status, rb_reduce_row *reduce_out, rb_norm_row *norm_out,
                                rb_hit_row **rows, uint64_t *n_rows, rb_reduce_row **stats, rb_counters *counters);
int rb_host_break_stats_text(rb_ctx *ctx, uint64_t n_rec, const uint8_t *text, uint64_t text_bytes, const uint64_t *cig_off,
                             const uint64_t *cig_end, const uint64_t *t_st, const uint64_t *t_en, const uint64_t *q_st, const uint64_t *q_en,
                             const uint8_t *strand, uint32_t max_size, int bsearch_policy, uint8_t *cig_status, rb_reduce_row *reduce_out,
                             rb_norm_row *norm_out, rb_hit_row **rows, uint64_t *n_rows, rb_reduce_row **stats, rb_counters *counters);
/* `rb break-paf --max-size N in.paf [| rb orient -] [| rb filter --paired-len L --aln A --query Q -]` (rb_host_break_pairs_text) and the same
 * with `| rb stats --paf [--qbed] -` behind it (rb_host_break_pairs_stats_text) as ONE device pipeline: the pieces are never printed or read
 * back.  Arguments as rb_host_break_text / rb_host_break_stats_text, then those of rb_dev_pairs_rows: rec_key / rec_q_len [n_rec] (the caller's
 * interning of the records' (target name, query name) pairs, and column 2), n_keys, mode, the three thresholds; key_flip [n_keys] OUT (host).
 * Flow: parse, rb_dev_scan_records, rb_dev_break in descriptor mode, rb_dev_pairs_rows on the rows where they lie, then rb_dev_format_cigars or
 * rb_dev_stats_rows on the kept rows as in the plain wrappers.  The rows that come back are the KEPT rows, dense, in row order, flipped keys'
 * q_st / q_en rewritten; the caller appends + / - to the query name and turns the strand by key_flip[rec_key[rows[k].rec]].
 * *declined != 0 (the call returns RB_OK, no rows come back): rb_pairs_info.declined of the call -- the caller replays the file on the record
 * route. */
int rb_host_break_pairs_text(rb_ctx *ctx, uint64_t n_rec, const uint8_t *text, uint64_t text_bytes, const uint64_t *cig_off,
                             const uint64_t *cig_end, const uint64_t *t_st, const uint64_t *t_en, const uint64_t *q_st, const uint64_t *q_en,
                             const uint8_t *strand, uint32_t max_size, int bsearch_policy, uint8_t *cig_status, rb_reduce_row *reduce_out,
                             rb_norm_row *norm_out, rb_hit_row **rows, uint64_t *n_rows, uint64_t **row_text_off, uint8_t **row_text,
                             rb_counters *counters, const uint32_t *rec_key, const uint64_t *rec_q_len, uint64_t n_keys, uint32_t mode,
                             uint64_t paired_len, uint64_t min_aln, uint64_t min_query, uint8_t *key_flip, int *declined);
int rb_host_break_pairs_stats_text(rb_ctx *ctx, uint64_t n_rec, const uint8_t *text, uint64_t text_bytes, const uint64_t *cig_off,
                                   const uint64_t *cig_end, const uint64_t *t_st, const uint64_t *t_en, const uint64_t *q_st, const uint64_t *q_en,
                                   const uint8_t *strand, uint32_t max_size, int bsearch_policy, uint8_t *cig_status, rb_reduce_row *reduce_out,
                                   rb_norm_row *norm_out, rb_hit_row **rows, uint64_t *n_rows, rb_reduce_row **stats, rb_counters *counters,
                                   const uint32_t *rec_key, const uint64_t *rec_q_len, uint64_t n_keys, uint32_t mode, uint64_t paired_len,
                                   uint64_t min_aln, uint64_t min_query, uint8_t *key_flip, int *declined);
/* `rb orient [--scaffold] in.paf` and `rb filter --paired-len L --aln A --query Q in.paf` on the records of a file: the first eleven arguments as
 * every text entry point, then those of rb_dev_pairs_records (rec_key / rec_q_len [n_rec]: the caller's interning of the (target name, query
 * name) pairs, and column 2).  Flow: parse, rb_dev_scan_records (reduce_out [n_rec]: Paf::from_file's check_integrity, nmatch and aln_len),
 * rb_dev_pairs_records with room for every record, rb_dev_format_cigars over the KEPT records only -- one item per kept record, in record order.
 * Out: cig_status [n_rec]; reduce_out [n_rec]; *kept [*n_kept] the kept records' indices, ascending (malloc'ed, rb_host_free); q_st_out /
 * q_en_out [n_rec] the records' query coordinates, flipped where their key is; key_flip / key_order [n_keys]; *row_text and *row_text_off
 * [*n_kept + 1] (malloc'ed): kept record k's CIGAR is row_text[row_text_off[k] .. row_text_off[k + 1]).  The caller appends + / - to the query
 * name and turns the strand by key_flip[rec_key[r]]; --scaffold sorts an index array by (target name, key_order[rec_key[r]], q_st_out[r]).
 * A CIGAR that did not parse: RB_OK, cig_status says which, nothing else is produced.  *declined != 0 (RB_OK, no kept records and no text come
 * back; the columns and the key arrays are what the rules say): rb_pairs_info.declined -- the caller replays the file on the record route. */
int rb_host_pairs_text(rb_ctx *ctx, uint64_t n_rec, const uint8_t *text, uint64_t text_bytes, const uint64_t *cig_off, const uint64_t *cig_end,
                       const uint64_t *t_st, const uint64_t *t_en, const uint64_t *q_st, const uint64_t *q_en, const uint8_t *strand,
                       const uint32_t *rec_key, const uint64_t *rec_q_len, uint64_t n_keys, uint32_t mode, uint64_t paired_len, uint64_t min_aln,
                       uint64_t min_query, uint8_t *cig_status, rb_reduce_row *reduce_out, uint32_t **kept, uint64_t *n_kept, uint64_t *q_st_out,
                       uint64_t *q_en_out, uint8_t *key_flip, uint64_t *key_order, uint64_t **row_text_off, uint8_t **row_text, int *declined);
/* `rb break-paf --max-size N in.paf | rb liftover --bed W -` (and the same with `| rb stats --paf` behind it) as ONE device pipeline: the
 * pieces are never printed, read back, parsed or uploaded.  Arguments as rb_host_liftover_text / rb_host_liftover_stats_text plus max_size;
 * RB_LIFT_QBED is refused (RB_E_INVALID).  Flow: parse, rb_dev_scan_records, rb_dev_break in descriptor mode, rb_dev_rows_to_batch (the
 * second command's Paf::from_file), rb_dev_scan_records on the pieces (its aligned_pairs), a plan over the pieces -- contigs in order of
 * first appearance among the PIECES --, rb_dev_liftover in descriptor mode on the piece batch, then rb_dev_format_cigars or
 * rb_dev_stats_rows as in the plain wrappers.  The first clip call's rows, descriptors and workspace are freed before the second call
 * allocates its own: the peak is one liftover call plus the piece batch.
 * On return rows[k].rec is the PARENT record's index in the input (names, lengths and mapq come from there), (*row_piece)[k] the piece's
 * ordinal among all pieces (malloc'ed, rb_host_free), rows[k].win the window; a piece's own id is empty (a record read from a file).
 * reduce_out / norm_out are the INPUT records' rows (the first command's checks).
 * *declined != 0 (the call returns RB_OK, nothing else is promised; free what came back): the caller replays the file on the record
 * route -- a status that is not RB_ST_OK in the input's reduce or norm rows, a panic status in a row of either clip call or in a piece's
 * norm row, a piece whose norm row has RB_F_STRIPPED (its own id would be _TO.<lead>.<trail>), or rb_pieces_info.declined. */
int rb_host_break_liftover_text(rb_ctx *ctx, uint64_t n_rec, const uint8_t *text, uint64_t text_bytes, const uint64_t *cig_off,
                                const uint64_t *cig_end, const uint64_t *t_st, const uint64_t *t_en, const uint64_t *q_st, const uint64_t *q_en,
                                const uint8_t *strand, const uint32_t *contig, uint64_t n_win, const uint32_t *w_contig, const uint64_t *w_st,
                                const uint64_t *w_en, uint32_t max_size, int bsearch_policy, uint8_t *cig_status, rb_reduce_row *reduce_out,
                                rb_norm_row *norm_out, rb_hit_row **rows, uint64_t *n_rows, uint64_t **row_text_off, uint8_t **row_text,
                                rb_counters *counters, uint32_t **row_piece, int *declined);
int rb_host_break_liftover_stats_text(rb_ctx *ctx, uint64_t n_rec, const uint8_t *text, uint64_t text_bytes, const uint64_t *cig_off,
                                      const uint64_t *cig_end, const uint64_t *t_st, const uint64_t *t_en, const uint64_t *q_st, const uint64_t *q_en,
                                      const uint8_t *strand, const uint32_t *contig, uint64_t n_win, const uint32_t *w_contig, const uint64_t *w_st,
                                      const uint64_t *w_en, uint32_t max_size, int bsearch_policy, uint8_t *cig_status, rb_reduce_row *reduce_out,
                                      rb_norm_row *norm_out, rb_hit_row **rows, uint64_t *n_rows, rb_reduce_row **stats, rb_counters *counters,
                                      uint32_t **row_piece, int *declined);
/* rb_dev_stats_rows on host arrays (the rows and clips of rb_host_liftover / rb_host_break, whose out_ops are dense and whose rows never
 * carry RB_HIT_DESCRIPTOR; descriptor rows work too, through ops / op_off): uploads, runs, downloads.  stats [n_rows] caller-allocated. */
int rb_host_stats_rows(rb_ctx *ctx, uint64_t n_rec, const uint32_t *ops, const uint64_t *op_off, const rb_hit_row *rows, uint64_t n_rows,
                       const uint32_t *out_ops, uint64_t n_out, rb_reduce_row *stats);
int rb_host_scan_text(rb_ctx *ctx, uint64_t n_rec, const uint8_t *text, uint64_t text_bytes, const uint64_t *cig_off, const uint64_t *cig_end,
                      const uint64_t *t_st, const uint64_t *t_en, const uint64_t *q_st, const uint64_t *q_en, const uint8_t *strand,
                      uint8_t *cig_status, rb_reduce_row *reduce_out, rb_norm_row *norm_out);

/* ---- stats of ALIGNMENT records (`rb stats` on SAM / BAM, main.rs:60-77): MD strings and query spans -------------------------- *
 *
 * rb_dev_parse_md   <- bamstats::parse_md_for_stats (bamstats.rs:48-79) for n strings: the regex (\d+)|([A-Z])|(\^[A-Z]+) applied left
 *                      to right, restated as runs: every maximal digit run adds its value; every maximal run of A-Z whose preceding
 *                      byte (inside the string) is '^' is one deletion event of that many bases; every other A-Z byte is one mismatch;
 *                      every other byte -- a lone '^', lower case, anything else -- is skipped.  Sums wrap in u32.
 *     text      device bytes that hold the strings (the `MD:Z:` values, without the tag); 16-byte aligned.  SLACK: the call reads whole
 *               aligned 16-byte groups that hold at least one byte of a string, so text must be readable up to the next multiple of 16
 *               behind the last string's end; bytes outside a string are never looked at, whatever they are.
 *     md_off    [n] start of every string;  md_end [n] its end (an end at or in front of the start: the empty string, nothing is read)
 *     out       [4 n] OUT u32, 16-byte aligned: match_count, mismatch_count, deletion events, deletion bases of string r at out[4 r ..]
 *     status    [n] OUT  RB_MD_OK, or RB_MD_UNUSUAL: a digit run of ten or more digits (zero padded, or past u32) -- not decided on
 *               the device, as rb_dev_parse_cigars does with such lengths; out[4 r ..] is then four zeros, parse the string on the host
 *     Enqueues on the context's stream, does not synchronise.  n == 0 is valid.  Writes out[0 .. 4 n) and status[0 .. n), nothing else.
 *     Two calls on the same input write the same bytes.
 * rb_md_shape: the kernel's thresholds, for tests (no device needed): out[0] = bytes per step of a row of 16 lanes, out[1] = the
 *     longest string a row takes (longer ones are walked by the whole wavefront), out[2] = bytes per step of the wavefront.
 * rb_host_parse_md: the same on HOST arrays (text [text_bytes], no slack or alignment asked of it): uploads, runs, downloads.
 *
 * rb_dev_aln_stats  <- bamstats::cigar_stats (bamstats.rs:129-142, :190-207) minus the names, for the n = batch->n_rec alignments of a
 *                      batch: one rb_aln_row each.
 *     batch        only ops and op_off [n + 1] are read (aligned packed ops, as every kernel takes them); of a record's ops a few at both
 *                  ends: leading H / P, and from the last op back to the last M / = / X
 *     reduce_rows  [n] what rb_dev_scan_records wrote for that batch with all coordinates zero (their status is therefore not looked at)
 *     pos [n] i64 0-based leftmost position;  flag [n] u32 (only bit 16 is read);  l_seq [n] u32 (0 for a SEQ of `*`)
 *     md [4 n], md_status [n]  the outputs of rb_dev_parse_md, record r's at [4 r ..] / [r];  has_md [n] u8, != 0: the record has an MD tag.
 *                  has_md NULL: no record has one (md and md_status may then be NULL too); md_status NULL: all RB_MD_OK
 *     rows [n] OUT r_en = pos + t_bases;  q_st = leading H + leading S (also H S);  q_en = leading H + 1 + (q_bases - trailing S / I - 1);
 *                  q_len = leading H + l_seq + trailing H;  with flag & 16: q_st, q_en = q_len - q_en, q_len - q_st;  the seven counters
 *                  and three identities of the reduce row -- unless equal == 0 && matches > 0 and the record has an MD: then equal =
 *                  md[0], diff = md[1] and the identities are recomputed from them;  flags = RB_ALN_WARN_M for matches > 0 without MD
 *                  (the reference's warning);  status, in the reference's order of checks:
 *                    RB_ALN_PANIC_DEL_FIRST  rust-htslib read_pos: D / N before any op that describes read sequence
 *                    RB_ALN_PANIC_HARDCLIP   ... H between operations
 *                    RB_ALN_PANIC_NONE       read_pos is None: the span ends in D / N, there is no M / = / X, or t_bases == 0
 *                    RB_ALN_MD_STATUS | s    the MD is needed and its md_status s is not RB_MD_OK (the host parses that string)
 *                    RB_ALN_PANIC_MD_ASSERT  md[0] + md[1] != diff (bamstats.rs:133)
 *                  A row whose status is not RB_ALN_OK is all zero otherwise.
 *     Enqueues on the context's stream, does not synchronise.  n == 0 is valid.  Reads no text: no slack.  Writes rows[0 .. n) only.
 * rb_host_aln_stats: the same on HOST arrays (ops / op_off as rb_host_scan_records takes them, reduce_rows as it returned them). */
enum { RB_MD_OK = 0, RB_MD_UNUSUAL = 3 };
enum { RB_ALN_OK = 0, RB_ALN_PANIC_DEL_FIRST = 32, RB_ALN_PANIC_HARDCLIP = 33, RB_ALN_PANIC_NONE = 34, RB_ALN_PANIC_MD_ASSERT = 35,
       RB_ALN_MD_STATUS = 64 };
enum { RB_ALN_WARN_M = 1 };
typedef struct rb_aln_row { /* 80 B */
    int64_t r_en, q_st, q_en, q_len;
    uint32_t equal, diff, ins, del, matches, ins_events, del_events;
    float id_by_all, id_by_events, id_by_matches;
    uint32_t status, flags;
} rb_aln_row;
void rb_md_shape(uint32_t out[3]);
int rb_dev_parse_md(rb_ctx *ctx, const uint8_t *text, const uint64_t *md_off, const uint64_t *md_end, uint64_t n, uint32_t *out /* [4 n] */,
                    uint8_t *status /* [n] */);
int rb_host_parse_md(rb_ctx *ctx, const uint8_t *text, uint64_t text_bytes, const uint64_t *md_off, const uint64_t *md_end, uint64_t n,
                     uint32_t *out, uint8_t *status);
int rb_dev_aln_stats(rb_ctx *ctx, const rb_batch_view *batch, const rb_reduce_row *reduce_rows, const int64_t *pos, const uint32_t *flag,
                     const uint32_t *l_seq, const uint32_t *md, const uint8_t *md_status, const uint8_t *has_md, rb_aln_row *rows);
int rb_host_aln_stats(rb_ctx *ctx, uint64_t n, const uint32_t *ops, const uint64_t *op_off, const rb_reduce_row *reduce_rows, const int64_t *pos,
                      const uint32_t *flag, const uint32_t *l_seq, const uint32_t *md, const uint8_t *md_status, const uint8_t *has_md,
                      rb_aln_row *rows);

/* ---- the records of a BAM stream (`rb stats in.bam`, main.rs:60-77): columns and packed ops from the inflated bytes ----------- *
 *
 * rb_dev_bam_records  <- htslib's bam_read1 bounds, its aux walk for MD:Z and CG:B,I, and its long-CIGAR convention, for n records
 *                        where they lie in the inflated stream.  BAM's CIGAR words are the packed words of this interface; the call
 *                        gathers them, from whatever byte the name's length leaves them at, into the aligned ops array.
 *     data      device bytes of the inflated BAM stream; 16-byte aligned.  SLACK: the call reads whole aligned dwords and 16-byte
 *               groups that hold at least one byte of a record, so data must be readable up to the next multiple of 16 behind the
 *               last record's end; no byte outside [rec_off[r], rec_off[r] + rec_len[r]) is looked at, whatever it is.
 *     rec_off   [n] the first byte behind record r's block_size field;  rec_len [n] u32 that block_size.  n counts ALL records,
 *               mapped or not.  The hop from record to record (one read each, a serial chain) and the end of the stream are the host's.
 *     One entry per input record, no compaction -- the columns as rb_dev_scan_records / rb_dev_parse_md / rb_dev_aln_stats take them:
 *     tid [n] i32, pos [n] i64 (sign-extended), flag [n] u32, l_seq [n] u32, has_md [n] u8,
 *     md_off / md_end [n] u64 into data (an empty MD: md_end == md_off with has_md = 1),
 *     op_off [n + 1] u64 exclusive prefix of ops per record, ops u32 (capacity ops_cap, 16-byte aligned), status [n] u8:
 *       RB_BAM_SHORT_BLOCK  block_size < 32
 *       RB_BAM_NO_FIT       32 + l_read_name + 4 n_cigar + (l_seq + 1) / 2 + l_seq > block_size (in 64 bits)
 *       RB_BAM_BAD_NAME     l_read_name == 0, or the name's last byte is not NUL
 *     checked in this order, for unmapped records too.  A record whose status is not RB_BAM_OK has zero in every other column and 0 ops.
 *     A record with flag & 4 has 0 ops, has_md = 0 and md_off = md_end = 0; tid, pos, flag and l_seq are reported.
 *     The aux walk runs while p + 3 <= block_size: A c C take 1 byte, s S 2, i I f 4; Z / H run to the first NUL, or to the record's end
 *     if there is none (an unterminated MD:Z is then the bytes up to the record's end); B stops the walk if its 5-byte head or its
 *     array (element size * count, in 64 bits) runs past the record; any other type byte stops it.  What was found before a stop
 *     counts.  The LAST MD:Z and the last CG:B,I win.  If a CG:B,I was found, n_cigar >= 1 and the first in-record word is S of length
 *     l_seq, the record's ops are the tag's `count` words (that can be more than 65535); otherwise the in-record words.  Op nibbles
 *     are copied as they are.
 *     TRUNCATION, as rb_dev_parse_cigars: the call returns RB_OK whatever ops_cap is, every column and op_off are exact whatever it
 *     is, nothing is written at or behind ops[ops_cap]: the caller detects a short ops[] by op_off[n] > ops_cap.  (bytes of data) / 4
 *     is always enough: every word is four bytes of a record.
 *     scratch   rb_bam_scratch_bytes(n) bytes.
 *     Enqueues on the context's stream, does not synchronise.  n == 0 is valid (op_off[0] = 0).  Writes its outputs and scratch,
 *     nothing else.  Two calls on the same input write the same bytes.
 * rb_bam_shape: the kernels' thresholds, for tests (no device needed): out[0 .. 2] = bytes per step of a row of 16 lanes in the search
 *     for a Z / H value's NUL, the longest aux area a row walks (longer ones take the whole wavefront), bytes per step of the
 *     wavefront; out[3 .. 5] = the same of the copy, in ops: per step of a row, the longest CIGAR a row copies, per step of the wavefront.
 * rb_host_bam_records: the same on HOST arrays (data [data_bytes], no slack or alignment asked of it; every record must lie inside it;
 *     ops [ops_cap] caller-allocated): uploads, runs, downloads. */
enum { RB_BAM_OK = 0, RB_BAM_SHORT_BLOCK = 1, RB_BAM_NO_FIT = 2, RB_BAM_BAD_NAME = 3 };
size_t rb_bam_scratch_bytes(uint64_t n);
void rb_bam_shape(uint32_t out[6]);
int rb_dev_bam_records(rb_ctx *ctx, const uint8_t *data, const uint64_t *rec_off, const uint32_t *rec_len, uint64_t n, int32_t *tid, int64_t *pos,
                       uint32_t *flag, uint32_t *l_seq, uint8_t *has_md, uint64_t *md_off, uint64_t *md_end, uint64_t *op_off, uint32_t *ops,
                       uint64_t ops_cap, uint8_t *status, void *scratch);
int rb_host_bam_records(rb_ctx *ctx, const uint8_t *data, uint64_t data_bytes, const uint64_t *rec_off, const uint32_t *rec_len, uint64_t n,
                        int32_t *tid, int64_t *pos, uint32_t *flag, uint32_t *l_seq, uint8_t *has_md, uint64_t *md_off, uint64_t *md_end,
                        uint64_t *op_off, uint32_t *ops, uint64_t ops_cap, uint8_t *status);

/* ---- the per-read index of `rb nucfreq in.bam` (k_bamreads.hip): what bam_read_records keeps per record besides the columns ------ *
 *
 * rb_dev_bam_reads  <- the SEQ place, the (tid, pos) key, the running maximum of (tid, bam_endpos) over the reads the pileup admits
 *                      and the sortedness test of the pileup iterator, for the n records rb_dev_bam_records decoded.
 *     data, rec_off, rec_len, n   as given to rb_dev_bam_records (rec_len is not read).  data 16-byte aligned, slack as there.
 *     tid, pos, flag, op_off, ops, status   what rb_dev_bam_records wrote.  ops holds all op_off[n] words (a call that was cut short
 *               by its ops_cap is not an input), is 16-byte aligned and readable to the next multiple of 4 words behind the last op:
 *               the call reads whole aligned 16-byte groups that hold a word of a record.
 *     One entry per record, no compaction:
 *     seq_off [n] u64       the byte of data where the record's SEQ starts: rec_off + 32 + l_read_name + 4 * n_cigar_op with the
 *                           IN-RECORD n_cigar_op (behind the two in-record words of a CG:B,I record); 0 where status != RB_BAM_OK.
 *     start_key [n] u64     (uint64_t)(uint32_t)tid << 32 | min((uint64_t)pos, 0xFFFFFFFF): a negative pos saturates.
 *     end_key_pmax [n] u64  the INCLUSIVE prefix maximum over records 0 .. i of the same key of (tid, endpos) of the reads that enter
 *                           the pileup: tid >= 0, no flag of 0x4 | 0x100 | 0x200 | 0x400, status == RB_BAM_OK.
 *                           endpos = max(pos, 0) + ((flag & 4) || ref == 0 ? 1 : ref), ref = the 64-bit sum of the lengths of the
 *                           record's ops whose nibble is M, D, N, = or X.  A read that does not enter carries the value in front of
 *                           it; the value in front of record 0 is 0.
 *     first_unsorted  one u64: the smallest i >= 1 with start_key[i] < start_key[i - 1] && tid[i] >= 0 && pos[i] >= 0; ~0 if none.
 *     scratch   rb_bam_reads_scratch_bytes(n) bytes, 256-byte aligned.
 *     Enqueues on the context's stream, does not synchronise.  n == 0 is valid (first_unsorted = ~0).  Writes its outputs and scratch,
 *     nothing else.  Two calls on the same input write the same bytes, whatever the buffers held.  RB_E_INVALID, before anything is
 *     enqueued: a NULL pointer that is needed, data or ops misaligned, scratch misaligned.
 * rb_bam_reads_shape: {ops per step of a row of 16 lanes, the longest CIGAR a row sums (longer ones take the whole wavefront), ops per
 *     step of the wavefront, records per workgroup of the scan} (no device needed).  A workgroup of the scan's second level takes as
 *     many maxima as the first takes records: above out[3] * out[3] records a serial top level joins in.
 * rb_host_bam_reads: rb_host_bam_records and this call on HOST arrays: uploads, runs both, downloads every column of both.
 *     RB_E_INVALID if ops_cap is smaller than the records' ops. */
size_t rb_bam_reads_scratch_bytes(uint64_t n);
void rb_bam_reads_shape(uint32_t out[4]);
int rb_dev_bam_reads(rb_ctx *ctx, const uint8_t *data, const uint64_t *rec_off, const uint32_t *rec_len, uint64_t n, const int32_t *tid,
                     const int64_t *pos, const uint32_t *flag, const uint64_t *op_off, const uint32_t *ops, const uint8_t *status,
                     uint64_t *seq_off, uint64_t *start_key, uint64_t *end_key_pmax, uint64_t *first_unsorted, void *scratch);
int rb_host_bam_reads(rb_ctx *ctx, const uint8_t *data, uint64_t data_bytes, const uint64_t *rec_off, const uint32_t *rec_len, uint64_t n,
                      int32_t *tid, int64_t *pos, uint32_t *flag, uint32_t *l_seq, uint8_t *has_md, uint64_t *md_off, uint64_t *md_end,
                      uint64_t *op_off, uint32_t *ops, uint64_t ops_cap, uint8_t *status, uint64_t *seq_off, uint64_t *start_key,
                      uint64_t *end_key_pmax, uint64_t *first_unsorted);

/* ---- nucfreq: A/C/G/T counts at every covered reference position -----------------
 *
 * rb_dev_nucfreq  <- nucfreq::nucfreq (nucfreq.rs:61-95) over the reads nucfreq::region_nucfreq fetches (:111-125),
 *                    for all the 10 kb pieces main.rs:100-110 cuts the regions into, in one call.
 *   reads   BAM records in FILE ORDER (coordinate sorted: (tid, pos) non-decreasing, unplaced reads with tid -1 last):
 *           ops / op_off  the CIGAR words (BAM's encoding is the packed encoding of this ABI; the host resolves the CG:B,I
 *                         long-cigar convention as htslib does) and their exclusive prefix [n_reads + 1]
 *           seq / seq_off 4-bit bases exactly as in the BAM record (=ACMGRSVTWYHKDBN, high nibble first), read i starting at
 *                         byte seq_off[i] (any byte); seq itself 4-byte aligned and readable for 32 bytes past the last read
 *                         (the kernel fetches 16 bytes at a time);  l_seq bases per read;  tid, pos (0-based leftmost), flag
 *   regions rg_tid / rg_st / rg_en [n_regions]  half-open, 0-based; out_off [n_regions + 1] = exclusive prefix of en - st
 *           (n_positions = out_off[n_regions]); regions may overlap, each is computed on its own
 *   counts  OUT [4 * n_positions] u32: A, C, G, T at position rg_st[r] + k -> counts[4 * (out_off[r] + k) ..].  Bit 31 of the A
 *           word (RB_NF_COVERED) is set where the pileup reports the position at all (some read that passes the flag
 *           filter covers it, deletions and reference skips included): the reference prints only those positions
 *   read_status OUT [n_reads] rb_read_status.  FILTERED = tid < 0 or a flag of htslib's default pileup mask (UNMAP |
 *           SECONDARY | QCFAIL | DUP).  BAD_CIGAR = htslib's cursor would assert (no reference-consuming op, a lone op that
 *           is not M/=/X, a zero-length M/D/N/=/X) or the spans do not fit 31 bits.  SEQ_SHORT = a counted base lies past
 *           l_seq (the reference panics on the index).  Reads that are not OK contribute nothing.
 *   counters OUT: max_depth (reads covering one position, deletions included), n_covered, n_bad, unsorted, n_dropped,
 *           cap_overflow.  htslib's pileup (bam_plp_push) drops a read that starts where the iterator stands while more than
 *           maxcnt = 8000 reads are buffered; that rule is restated on the device per region (= per fetch of the reference),
 *           oracle/rb_oracle.c rbo_nucfreq holds the same restatement: n_dropped counts the (region, read) pairs it removed.
 *           cap_overflow = 1 when the bookkeeping of that rule did not fit (more than 15360 reads buffered at once, or regions
 *           deeper than the cap overlapping each other more than 64-fold): the counts are then not the reference's.  The same
 *           goes for max_depth > 65535 (16-bit counters).  rb_host_nucfreq returns RB_E_INVALID for all three, and for
 *           unsorted input.
 *   ws      rb_nucfreq_workspace_bytes(n_reads, n_regions, n_positions) bytes, 256-byte aligned
 */
typedef struct {
    uint64_t n_reads;
    const uint32_t *ops;
    const uint64_t *op_off;
    const uint8_t *seq;
    const uint64_t *seq_off;
    const uint32_t *l_seq;
    const int32_t *tid;
    const int64_t *pos;
    const uint32_t *flag;
} rb_reads_view;
enum rb_read_status { RB_RD_OK = 0, RB_RD_FILTERED = 1, RB_RD_BAD_CIGAR = 2, RB_RD_SEQ_SHORT = 3 };
typedef struct {
    uint64_t max_depth, n_covered, n_bad, unsorted, n_dropped, cap_overflow;
} rb_nucfreq_counters;
#define RB_NF_COVERED 0x80000000u
#define RB_NF_DEPTH_CAP 8000u /* htslib bam_plp_init: maxcnt */
size_t rb_nucfreq_workspace_bytes(uint64_t n_reads, uint64_t n_regions, uint64_t n_positions);
int rb_dev_nucfreq(rb_ctx *ctx, const rb_reads_view *reads, uint64_t n_regions, const int32_t *rg_tid, const uint64_t *rg_st,
                   const uint64_t *rg_en, const uint64_t *out_off, uint64_t n_positions, uint32_t *counts, uint32_t *read_status,
                   rb_nucfreq_counters *counters, void *ws, size_t ws_bytes);
/* host-buffer form: uploads ops[op_off[0] .. op_off[n_reads]) and the sequence bytes the reads span, runs, downloads.
 * counts [4 * sum(en - st)] and read_status [n_reads] are caller-allocated; read_status may be NULL */
int rb_host_nucfreq(rb_ctx *ctx, const rb_reads_view *reads, uint64_t n_regions, const int32_t *rg_tid, const uint64_t *rg_st,
                    const uint64_t *rg_en, uint32_t *counts, uint32_t *read_status, rb_nucfreq_counters *counters);
/* resident-reads form: rb_host_nucfreq, except that every pointer of reads is DEVICE memory and nothing of the reads is uploaded.
 * ops and seq are the caller's bases, indexed by ABSOLUTE op_off / seq_off (the columns of rb_dev_bam_records / rb_dev_bam_reads, seq =
 * the stream itself); the other arrays may be interior pointers (column base + i0) for the slice [i0, i0 + n_reads), op_off with
 * n_reads + 1 entries.  MEMORY: seq is 4-byte aligned, and 32 readable bytes lie behind the last read's SEQ (a stream buffer is
 * allocated with that slack).  Regions, counts, read_status and counters are HOST memory as there; the refusals are the same. */
int rb_devreads_nucfreq(rb_ctx *ctx, const rb_reads_view *reads, uint64_t n_regions, const int32_t *rg_tid, const uint64_t *rg_st,
                        const uint64_t *rg_en, uint32_t *counts, uint32_t *read_status, rb_nucfreq_counters *counters);

/* ---- nucfreq: the lines printed on the device (k_nftext.hip) ----------------------------------------------------------
 *
 * rb_dev_nucfreq_text  <- impl Display for Nucfreq (nucfreq.rs:17-33) and the --small lines (nucfreq.rs:148-150), one line per
 *                         covered position, from the counts where rb_dev_nucfreq left them.
 *   counts    DEVICE, 16-byte aligned: the output of rb_dev_nucfreq, four u32 per position, RB_NF_COVERED in bit 31 of the A word
 *   segments  n_seg of them (below 2^32), described by seven HOST arrays of n_seg entries that are consumed before the call returns:
 *             segment s covers the positions seg_pos[s] + k, k < seg_n[s], whose counts start at counts[4 * (seg_cnt[s] + k)].
 *             Segments are independent: they may overlap in counts, and seg_cnt need not ascend.  A segment's prefix is
 *             strings[pre_off[s] .. + pre_len[s]), its suffix strings[suf_off[s] .. + suf_len[s]); strings is DEVICE memory.
 *             (The segment tables are a few words per print piece and the call has to look at them -- the refusals below, the launch
 *             size --: as host arrays it does so without waiting for the device.)
 *   text      Only positions whose A word has RB_NF_COVERED set make a line, in position order.
 *             RB_NFT_FULL:  prefix dec(p) TAB dec((uint32_t)(p + 1)) TAB dec(A & 0x7fffffff) TAB dec(C) TAB dec(G) TAB dec(T) suffix
 *             RB_NFT_SMALL: dec(largest of the four) TAB dec(second largest) LF; prefix and suffix are not looked at, strings and
 *                           their four arrays may be NULL
 *             The header lines (`#chr\tstart...`, `#name\tpos\tid`) are the caller's: seg_first says where the second kind goes.
 *   outputs   DEVICE: seg_text_off [n_seg + 1] exclusive prefix of the segments' bytes; seg_first [n_seg] the first covered position
 *             of the segment, ~0 if it has none; seg_lines [n_seg] its lines; text (16-byte aligned; NULL: a sizes-only call) the
 *             segments' lines back to back with no padding: a segment starts at the byte the one in front ended on.
 *   scratch   DEVICE, rb_nucfreq_text_scratch_bytes(n_seg, sum of seg_n) bytes, 256-byte aligned
 *   CONTRACT  The call enqueues on the context's stream and does not wait for it (the upload of the segment tables goes through the
 *             context's page-locked chunks, as every rb_dev_upload does, and can wait for an earlier upload's copy to leave its chunk:
 *             never for a kernel).  It writes its outputs and its scratch and nothing
 *             else; two calls on the same input write the same bytes, whatever outputs and scratch held before.
 *             TRUNCATION: the call returns RB_OK whatever text_cap is, and the three segment arrays are exact whatever it is: the caller
 *             detects a short text[] by seg_text_off[n_seg] > text_cap.  Nothing is written at or behind text[text_cap].  Below it
 *             every segment that ends at or in front of the last 16-byte boundary <= text_cap is printed whole; of the others any
 *             byte may be missing (a 16-byte group that would reach behind text_cap is left out whole), and a byte that is there is
 *             the right one.
 *             RB_E_INVALID, before anything is enqueued: seg_pos[s] + seg_n[s] > 2^32; a prefix or suffix longer than 255 bytes
 *             (RB_NFT_FULL); a mode that is neither; a NULL pointer that is needed; counts, text or scratch misaligned.
 *             n_seg == 0 and seg_n[s] == 0 are valid.
 * rb_nucfreq_text_shape: {positions per wavefront step, positions per workgroup, longest prefix, longest suffix} (no device needed).
 * rb_host_nucfreq_text: rb_host_nucfreq with the lines instead of the counts.  Reads and regions as there; the segments as above with
 *             seg_cnt relative to the layout rb_host_nucfreq gives counts (region r at the sum of en - st of the regions in front),
 *             and strings a HOST array of strings_bytes bytes.  The counts never leave the device.  The refusals are those of
 *             rb_host_nucfreq (unsorted, cap_overflow, depth > 65535: RB_E_INVALID, nothing is handed to sink); read_status [n_reads]
 *             and counters come back as there.  The text is printed in runs of whole segments of at most 1 GiB and handed to sink in
 *             segment order: segments [first_seg, first_seg + n_seg), seg_text_off [n_seg + 1] relative to text, seg_first [n_seg]; the
 *             three pointers are valid until sink returns.  A single segment of more than 1 GiB of text gets a slab of its own size.
 *             (RB_DEBUG_NFT_SLAB=<bytes> in the environment lowers the 1 GiB: the tests' way to several slabs at a small size.) */
enum { RB_NFT_FULL = 0, RB_NFT_SMALL = 1 };
size_t rb_nucfreq_text_scratch_bytes(uint64_t n_seg, uint64_t n_positions);
void rb_nucfreq_text_shape(uint32_t out[4]);
int rb_dev_nucfreq_text(rb_ctx *ctx, const uint32_t *counts, uint64_t n_seg, const uint64_t *seg_cnt, const uint64_t *seg_pos,
                        const uint32_t *seg_n, const uint8_t *strings, const uint32_t *pre_off, const uint32_t *pre_len,
                        const uint32_t *suf_off, const uint32_t *suf_len, int mode, uint64_t *seg_text_off, uint64_t *seg_first,
                        uint64_t *seg_lines, uint8_t *text, uint64_t text_cap, void *scratch);
int rb_host_nucfreq_text(rb_ctx *ctx, const rb_reads_view *reads, uint64_t n_regions, const int32_t *rg_tid, const uint64_t *rg_st,
                         const uint64_t *rg_en, uint64_t n_seg, const uint64_t *seg_cnt, const uint64_t *seg_pos, const uint32_t *seg_n,
                         const uint8_t *strings, uint64_t strings_bytes, const uint32_t *pre_off, const uint32_t *pre_len,
                         const uint32_t *suf_off, const uint32_t *suf_len, int mode, uint32_t *read_status, rb_nucfreq_counters *counters,
                         void (*sink)(void *user, uint64_t first_seg, uint64_t n_seg, const uint64_t *seg_text_off,
                                      const uint64_t *seg_first, const uint8_t *text),
                         void *user);
/* resident-reads form: rb_host_nucfreq_text with reads a DEVICE view under the memory contract of rb_devreads_nucfreq; segments, strings,
 * read_status, counters and sink stay HOST-side; refusals, slabs and RB_DEBUG_NFT_SLAB as there. */
int rb_devreads_nucfreq_text(rb_ctx *ctx, const rb_reads_view *reads, uint64_t n_regions, const int32_t *rg_tid, const uint64_t *rg_st,
                             const uint64_t *rg_en, uint64_t n_seg, const uint64_t *seg_cnt, const uint64_t *seg_pos, const uint32_t *seg_n,
                             const uint8_t *strings, uint64_t strings_bytes, const uint32_t *pre_off, const uint32_t *pre_len,
                             const uint32_t *suf_off, const uint32_t *suf_len, int mode, uint32_t *read_status, rb_nucfreq_counters *counters,
                             void (*sink)(void *user, uint64_t first_seg, uint64_t n_seg, const uint64_t *seg_text_off,
                                          const uint64_t *seg_first, const uint8_t *text),
                             void *user);

/* ---- verification aid (tests, bench; not a reference function): digest of hit rows and their clipped CIGARs ---------------
 * *digest += sum over i < n_rows of mix(row i) * (2 * (row_base + i) + 1), wrapping u64 (the caller zeroes *digest).  mix covers
 * rec + rec_base, win, status and -- for RB_ST_OK rows -- the INSIDE flag, out_n, the coordinates, nmatch, aln_len and every op of
 * the clip in order.  It does NOT cover out_off, nor how the clip is stored: a descriptor row (RB_HIT_DESCRIPTOR) is expanded
 * through batch->ops / batch->op_off.  Two runs that produce the same records in the same order have the same digest wherever
 * the ops were placed, and the digests of contiguous record-range shards add up to the digest of the whole batch when each shard
 * passes the rows / records that precede it as row_base / rec_base (the 1/2/4/8-GPU determinism check of bench.py). */
int rb_dev_digest_rows(rb_ctx *ctx, const rb_batch_view *batch, const rb_hit_row *rows, uint64_t n_rows, const uint32_t *out_ops,
                       uint64_t row_base, uint64_t rec_base, uint64_t *digest);

/* ---- diagnostics: the box (bench.py's `box` block; not a reference function) ------------------------------------------- *
 * Moves the clip kernel's memory mix without its instructions: every wave reads a 20 KiB stretch of src[0 .. src_bytes) in the clip
 * kernel's access shape and writes it to dst0 (all of it) and dst1 (a fifth of it); both need src_bytes of room.  reps launches
 * back to back; *ms_out = mean time of one, *mhz_out (may be NULL) = the shader clock held meanwhile, from s_memtime / s_memrealtime
 * stamps around each wave's loop.  scatter != 0: the waves that run at the same time work 5 MB apart, all over the array (as the clip
 * kernel's do: its records run longest first), instead of side by side; 2 / 3: the same two orders with the other load shape (every
 * instruction covering 1 KiB of whole lines instead of 32 contiguous bytes per lane); + 4: the read side alone (no stores), + 8: the
 * write side alone (no loads). */
int rb_dev_box_probe(rb_ctx *ctx, const void *src, uint64_t src_bytes, void *dst0, void *dst1, int reps, int scatter, double *ms_out, double *mhz_out);

/* A buffer that will be WRITTEN at streaming rate (an output arena), placed by measurement: on MI355X the time of a launch that streams
 * its output into a buffer depends on which physical pages the buffer has (same process, same launch, the arena allocated four times
 * over: 9.10 / 9.17 / 9.25 / 11.04 ms; reads do not care).  Allocates up to `tries` candidates of `bytes` with rb_dev_alloc -- fewer
 * when the device lacks the room --, times a store sweep over each, returns the fastest in *out (free it with rb_dev_free) and gives
 * the others back.  sweep_ms (NULL or room for `tries` doubles): the time of each candidate's sweep, -1 where none was made;
 * *kept (may be NULL): the index of the one returned.  tries = 1 is rb_dev_alloc. */
int rb_dev_alloc_placed(rb_ctx *ctx, uint64_t bytes, int tries, void **out, double *sweep_ms, int *kept);
/* The same with the caller's own measure instead of the store sweep: score(candidate, user) is called once per candidate (nothing of
 * the library is locked meanwhile; it may launch on the context and must leave the device idle or its work ordered on the context's
 * stream) and returns a time -- the lowest wins, a negative one ends the search with RB_E_INVALID.  The measure that counts is the
 * launch the buffer is for: the sweep tells a 9.2 ms arena from an 11 ms one, not always a 9.9 ms one from a 10.1 ms one. */
int rb_dev_alloc_placed_by(rb_ctx *ctx, uint64_t bytes, int tries, double (*score)(void *candidate, void *user), void *user, void **out,
                           double *scores, int *kept);

/* ---- synthetic workload generator (bench and tests, not a reference function) -- *
 * Counter-based: ops of record r depend only on (seed, first_record + r, op index).  The host and
 * device versions produce identical bytes.  n_ops per record comes from rb_synth_n_ops. */
uint32_t rb_synth_n_ops(uint64_t seed, uint64_t record, uint32_t lo, uint32_t hi);
/* the "imbalance" shape of SURVEY.md 8(d): log-normal (mu = ln 2000, sigma = 1.35) clipped to [31, 80000] ops, forced odd */
uint32_t rb_synth_n_ops_lognormal(uint64_t seed, uint64_t record);
void rb_synth_fill_ops_host(uint64_t seed, uint64_t first_record, uint64_t n_rec, const uint64_t *op_off, uint32_t *ops);
int rb_dev_synth_fill_ops(rb_ctx *ctx, uint64_t seed, uint64_t first_record, uint64_t n_rec, const uint64_t *op_off_dev,
                          uint32_t *ops_dev);

#ifdef __cplusplus
}
#endif
#endif /* RUSTYBAM_AMD_H */
