// rb_launch.h -- the launch interface between the host side of the library (capi.hip) and the kernel translation units: every
// kernel's parameter block and every rb_launch_* entry point and cross-TU helper, declared once and included by both sides.
// (rb_lift_params: rb_lift.h; rb_trim_params: rb_trim.h.)  Host declarations only: no device code lives here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rustybam_amd.h"

struct rb_lift_params;
struct rb_trim_params;
struct nf_read;  // k_nucfreq.hip
struct nf_tdesc; // k_nucfreq.hip

// ---- k_records.hip: K1, the per-record scan ----
struct rb_scan_params {
    uint64_t n_rec;
    const uint32_t *ops;
    const uint64_t *op_off;
    const uint64_t *t_st, *t_en, *q_st, *q_en;
    const uint8_t *strand;
    rb_reduce_row *reduce_rows;
    rb_norm_row *norm_rows;
    // list mode (fused liftover): only the records list[0 .. *n_list) are scanned
    const uint32_t *list;
    const uint64_t *n_list;
};
extern "C" hipError_t rb_launch_scan_records(const rb_scan_params *p, hipStream_t stream);
extern "C" hipError_t rb_launch_scan_rows(const rb_scan_params *p, void *long_buf, hipStream_t stream);
extern "C" hipError_t rb_launch_peek_norm(const rb_scan_params *p, hipStream_t stream);

// ---- k_liftover.hip, k_liftover_brk.hip, k_liftover_list.hip, k_tile.hip: the clip kernels ----
extern "C" hipError_t rb_launch_count_and_scan(const rb_lift_params *p, uint64_t *block_sums, bool do_count, hipStream_t stream);
extern "C" hipError_t rb_launch_exclusive_scan(uint64_t *v, uint64_t n, uint64_t *block_sums, uint64_t *total_out, hipStream_t stream);
extern "C" size_t rb_scan_block_sums_count(uint64_t n_rec);
extern "C" hipError_t rb_launch_make_jobs(const rb_lift_params *p, hipStream_t stream);
extern "C" hipError_t rb_launch_liftover_stream(const rb_lift_params *p, hipStream_t stream);
extern "C" hipError_t rb_launch_liftover_tail(const rb_lift_params *p, hipStream_t stream);
extern "C" hipError_t rb_launch_liftover_stream_list(const rb_lift_params *p, hipStream_t stream);
extern "C" hipError_t rb_launch_liftover_stream_brk(const rb_lift_params *p, unsigned blocks, hipStream_t stream); // k_liftover_brk.hip, called by rb_launch_liftover_stream
extern "C" hipError_t rb_launch_liftover_tiles(const rb_lift_params *p, hipStream_t stream);
extern "C" uint32_t rb_tile_max_ops(void);
extern "C" uint32_t rb_tile_max_records(void);
extern "C" hipError_t rb_launch_break_gather(const rb_lift_params *p, hipStream_t stream);
extern "C" hipError_t rb_launch_break_declined(const rb_lift_params *p, hipStream_t stream);
extern "C" hipError_t rb_launch_break_list_declined(const rb_lift_params *p, hipStream_t stream);

// ---- k_misc.hip: break-paf pieces, invert, synthetic ops, digest, clip compaction, the box probe ----
struct rb_break_params {
    uint64_t n_rec;
    const uint32_t *ops;
    const uint64_t *op_off;
    const rb_norm_row *norm;
    const uint32_t *sched;
    uint64_t *hit_off;
    uint64_t *x_st, *x_en;
    uint64_t rows_cap;
    uint32_t max_size;
    int fill; // 0: count pieces; 1: write the windows of every record (or, with redo_only, of the records the collect pass gave up on);
              // 2 (collect): count AND keep the windows, in LDS while the record streams, then in tmp[] at a slot from tmp_cursor
    int redo_only;
    uint2 *tmp;                    // [rows_cap] (start, end) of a piece relative to the record's t_st
    uint64_t *tmp_off;             // [n_rec] where the record's pieces sit in tmp[]; ~0 = not kept (more than RB_BP_CAP pieces, or no room)
    unsigned long long *tmp_cursor; // one bump cursor per arena, 128 bytes apart (a single cursor would serialise every record at one L2 line)
    uint32_t n_arena;
    uint64_t arena_cap;             // slots of tmp[] per arena
    // list mode (break-paf in one walk: the records its clip kernel declined): wave w takes record list[w], w < *n_list
    const uint32_t *list;
    const unsigned long long *n_list;
};
struct rb_swap_params { // rb_k_swap: ops -> out_ops (disjoint arrays); rb_k_swap_inplace: ops rewritten where they lie, out_ops not read
    uint64_t n_rec;
    const uint32_t *ops;
    const uint64_t *op_off;
    const uint8_t *strand;
    uint32_t *out_ops;
};
struct rb_digest_params {
    const uint32_t *ops;     // the batch's packed ops (descriptor rows are expanded through them)
    const uint64_t *op_off;
    const rb_hit_row *rows;
    uint64_t n_rows;
    const uint32_t *out_ops;
    uint64_t row_base, rec_base;
    unsigned long long *digest;
};
struct rb_compact_params {
    uint64_t n_rows;
    rb_hit_row *rows;
    const uint32_t *src; // out_ops of the clip call
    uint64_t *off;       // [n_rows + 1] words per row, then their exclusive prefix
    uint32_t *dst;
    int fill;
};
extern "C" hipError_t rb_launch_break_pieces(const rb_break_params *p, hipStream_t stream);
extern "C" hipError_t rb_launch_break_place(const rb_break_params *p, hipStream_t stream);
extern "C" hipError_t rb_launch_swap(const rb_swap_params *p, hipStream_t stream);
extern "C" hipError_t rb_launch_swap_inplace(const rb_swap_params *p, hipStream_t stream);
extern "C" hipError_t rb_launch_starts_check(const uint64_t *op_off, const rb_norm_row *norm, uint64_t n_rec, uint64_t n_ops, unsigned long long *bad,
                                             hipStream_t stream);
extern "C" hipError_t rb_launch_synth(uint64_t seed, uint64_t first_record, uint64_t n_rec, const uint64_t *op_off, uint32_t *ops, hipStream_t stream);
extern "C" hipError_t rb_launch_digest_rows(const rb_digest_params *p, hipStream_t stream);
extern "C" hipError_t rb_launch_compact_clips(const rb_compact_params *p, hipStream_t stream);
extern "C" hipError_t rb_launch_box_probe(const void *src, void *d0, void *d1, uint64_t n_stretch, uint32_t *stamps, int scatter, hipStream_t stream);

// ---- k_text.hip: CIGAR text ----
struct rb_parse_params {
    uint64_t n_rec;
    const uint8_t *text;      // all CIGAR strings, any layout
    const uint64_t *text_off; // [n_rec + 1] record r's string is text[text_off[r] .. text_end[r])
    const uint64_t *text_end; // [n_rec] (NULL: strings are back to back, end = text_off[r + 1])
    uint64_t *op_off;         // [n_rec + 1] counts (count pass) / offsets (fill pass)
    uint32_t *ops;
    uint64_t ops_cap;
    uint8_t *status;          // [n_rec] RB_TEXT_*
};
struct rb_format_params {
    uint64_t n_items;
    const uint32_t *ops;
    const uint32_t *ops_alt;   // second source: items whose first[] has bit 63 set index this array (NULL if unused)
    const uint64_t *first;     // [n_items] index of the item's first op in ops[] (bit 63: in ops_alt[])
    const uint32_t *count;     // [n_items] ops in the item (0 = empty text)
    const uint32_t *first_len; // [n_items] or NULL: != 0 replaces the length of the first op
    const uint32_t *last_len;  // [n_items] or NULL: != 0 replaces the length of the last op; a one-op item with both keeps first + last - len
    uint64_t *text_off;        // [n_items + 1] counts / offsets
    uint8_t *text;
    uint64_t text_cap;
    int plain_ops;             // != 0: the items of ops[] hold no continuation words (a batch the device parsed: rb_k_parse_cigars makes none)
};
extern "C" hipError_t rb_launch_parse_cigars(const rb_parse_params *p, bool fill, hipStream_t stream);
extern "C" hipError_t rb_launch_format_cigars(const rb_format_params *p, bool fill, hipStream_t stream);

// ---- k_trim.hip, k_trim4.hip, k_trim_pass.hip: trim-paf ----
struct rb_apply_params {
    uint64_t n_pairs;
    const uint32_t *left, *right;
    const rb_pair_row *rows;
    uint64_t *op_off;
    rb_norm_row *norm;
};
struct rb_gather_params {
    uint64_t n_rec;
    const uint32_t *ops;
    const uint64_t *op_off;
    const rb_norm_row *norm;
    uint64_t *new_off; // [n_rec + 1]: counts (fill == 0) then their exclusive prefix
    uint32_t *new_ops;
    int fill;
};
struct rb_tsel_params {
    uint64_t n_groups;
    const uint32_t *order;     // [n_rec] records stably sorted by query name
    const uint64_t *grp_off;   // [n_groups + 1] group g = order[grp_off[g] .. grp_off[g + 1])
    const rb_norm_row *norm;   // current coordinates / lengths of every record
    uint8_t *contained;        // [n_rec] by record: the flags of THIS pass (paf.rs:224: reset at every level)
    uint64_t *slot;            // [n_groups + 1] ops(left) + ops(right) of the group's pair (0: none); scanned in place: where its clips go
    uint64_t *has;             // [n_groups + 1] 1 for a group with a pair, else 0; scanned in place: the pair's dense slot
    uint32_t *cand;            // [2 n_groups] the chosen (left, right) records of each group
    uint64_t out_base;
    uint32_t *left, *right;    // dense outputs
    uint64_t *pair_out_off;
    rb_trim_pass *pass;
};
extern "C" hipError_t rb_launch_overlap_split(const rb_trim_params *p, hipStream_t stream);
extern "C" hipError_t rb_launch_overlap_split_quad(const rb_trim_params *p, int t, bool from_list, hipStream_t stream);
extern "C" size_t rb_trim_scratch_bytes(uint32_t blocks);
extern "C" hipError_t rb_launch_apply_pairs(const rb_apply_params *p, hipStream_t stream);
extern "C" hipError_t rb_launch_gather_records(const rb_gather_params *p, hipStream_t stream);
extern "C" hipError_t rb_launch_trim_select(const rb_tsel_params *p, uint64_t *block_sums, hipStream_t stream);
extern "C" hipError_t rb_launch_trim_check(const rb_pair_row *rows, uint64_t n_pairs, rb_trim_pass *pass, hipStream_t stream);

// ---- k_largest.hip: liftover --largest ----
struct rb_largest_params {
    const rb_hit_row *rows;
    uint64_t n_rows;
    const uint32_t *win_key; // [n_win] key of a row that is not INSIDE
    const uint32_t *rec_key; // [n_rec] key of an INSIDE row (NULL: such a row has a bad key)
    uint64_t n_keys;
    unsigned long long *best_span; // [n_keys + 1] zeroed; pass 1: the largest span of every key.  Behind pass 2 it is free again and holds
                                   // the compaction's counts (1: the key has a winner), then their exclusive prefix
    unsigned long long *best_row;  // [n_keys] zeroed; pass 2: 1 + the largest row index among the key's rows of that span (0: no row)
    uint64_t *sel;                 // [n_keys] OUT the winners' row indices, dense, in ascending key order
    unsigned long long *out;       // zeroed; [0] = n_sel, [1] = rows left out for their key
    uint32_t *worst_status;        // NULL, or zeroed: the largest status of RB_ST_PANIC_NOTFOUND and above among ALL rows (rb_host_liftover_largest_text)
};
extern "C" hipError_t rb_launch_largest(const rb_largest_params *p, uint64_t *block_sums, hipStream_t stream);
extern "C" hipError_t rb_launch_largest_rec_keys(const rb_norm_row *norm, uint64_t n_rec, uint32_t inside_key, uint32_t *rec_key, hipStream_t stream);
extern "C" hipError_t rb_launch_largest_gather(const rb_hit_row *rows, const uint32_t *out_ops, const uint64_t *sel, uint64_t n_sel, rb_hit_row *sel_rows,
                                               uint32_t *sel_desc, hipStream_t stream);

// ---- k_pairs.hip: orient / filter over hit rows, keyed by the records' (target, query) pair ----
struct rb_pairs_params {
    const rb_hit_row *rows;
    uint64_t n_rows;
    const uint32_t *rec_key;   // [n_rec]
    const uint64_t *rec_q_len; // [n_rec]
    const uint8_t *strand;     // [n_rec]
    uint64_t n_rec, n_keys;
    uint32_t mode;             // RB_PAIRS_ORIENT | RB_PAIRS_FILTER
    uint64_t paired_len, min_aln, min_query;
    unsigned long long *orient, *tspan, *fspan; // [n_keys] each, zeroed: the three sums (orient is an i64 in two's complement)
    uint64_t *cnt;             // [n_rows + 1]: 1 per kept row, then the exclusive prefix
    rb_hit_row *rows_out;
    uint64_t rows_cap;
    uint8_t *key_flip;         // [n_keys] OUT
    rb_pairs_info *info;       // zeroed
};
extern "C" hipError_t rb_launch_pairs(const rb_pairs_params *p, uint64_t *block_sums, hipStream_t stream);
extern "C" hipError_t rb_launch_pairs_desc(const rb_hit_row *rows, uint64_t n_rows, const uint32_t *out_ops, uint32_t *desc /* [4 * n_rows] */, hipStream_t stream);
extern "C" uint32_t rb_pairs_wave_rows(void);
extern "C" uint32_t rb_pairs_block_rows(void);
// the same over the RECORDS of a batch (rb_dev_pairs_records): the columns instead of rows, a fourth sum (order), the kept records' indices out
struct rb_pairs_rec_params {
    const uint64_t *t_st, *t_en, *q_st, *q_en; // [n_rec]
    const uint8_t *strand;     // [n_rec]
    const uint32_t *rec_key;   // [n_rec]
    const uint64_t *rec_q_len; // [n_rec]
    uint64_t n_rec, n_keys;
    uint32_t mode;             // RB_PAIRS_ORIENT | RB_PAIRS_FILTER
    uint64_t paired_len, min_aln, min_query;
    unsigned long long *orient, *tspan, *fspan, *order; // [n_keys] each, zeroed: the four sums
    uint64_t *cnt;             // [n_rec + 1]: 1 per kept record, then the exclusive prefix
    uint32_t *kept;            // [kept_cap] OUT
    uint64_t kept_cap;
    uint64_t *q_st_out, *q_en_out; // [n_rec] OUT, or both NULL
    uint8_t *key_flip;         // [n_keys] OUT
    uint64_t *key_order;       // [n_keys] OUT, or NULL
    rb_pairs_info *info;       // zeroed
};
extern "C" hipError_t rb_launch_pairs_records(const rb_pairs_rec_params *p, uint64_t *block_sums, hipStream_t stream);

// ---- k_hitstats.hip: stats of every hit row's clip ----
struct rb_hitstats_params {
    const uint32_t *ops;     // the batch's packed ops (descriptor rows point into them)
    const uint64_t *op_off;  // used as a table of starts only
    const rb_hit_row *rows;
    uint64_t n_rows;
    const uint32_t *out_ops;
    rb_reduce_row *stats;    // [n_rows] OUT
};
extern "C" hipError_t rb_launch_hitstats(const rb_hitstats_params *p, hipStream_t stream);

// ---- k_alnstats.hip: MD strings and query spans of alignment records ----
struct rb_md_params {
    uint64_t n;
    const uint8_t *text;    // 16-byte aligned, readable to the next multiple of 16 behind the last string
    const uint64_t *md_off; // [n] string r is text[md_off[r] .. md_end[r])
    const uint64_t *md_end; // [n]
    uint32_t *out;          // [4 n] OUT match_count, mismatch_count, deletion events, deletion bases (16-byte aligned)
    uint8_t *status;        // [n] OUT RB_MD_*
};
struct rb_alnstats_params {
    uint64_t n;
    const uint32_t *ops;
    const uint64_t *op_off;            // [n + 1]
    const rb_reduce_row *reduce_rows;  // [n] the record scan's rows (coordinates zero: their status is not looked at)
    const int64_t *pos;                // [n]
    const uint32_t *flag, *l_seq;      // [n]
    const uint32_t *md;                // [4 n] or NULL
    const uint8_t *md_status, *has_md; // [n] or NULL
    rb_aln_row *rows;                  // [n] OUT
};
extern "C" hipError_t rb_launch_parse_md(const rb_md_params *p, hipStream_t stream);
extern "C" hipError_t rb_launch_aln_stats(const rb_alnstats_params *p, hipStream_t stream);
extern "C" uint32_t rb_md_row_step(void);
extern "C" uint32_t rb_md_wave_step(void);
extern "C" uint32_t rb_md_row_max(void);

// ---- k_bam.hip: the records of an inflated BAM stream as columns and packed ops ----
struct rb_bam_params {
    uint64_t n;
    const uint8_t *data;     // 16-byte aligned, readable to the next multiple of 16 behind the last record
    const uint64_t *rec_off; // [n] the first byte behind the record's block_size field
    const uint32_t *rec_len; // [n] its block_size
    int32_t *tid;            // [n] OUT
    int64_t *pos;            // [n] OUT
    uint32_t *flag, *l_seq;  // [n] OUT
    uint8_t *has_md;         // [n] OUT
    uint64_t *md_off, *md_end; // [n] OUT places in data
    uint64_t *op_off;        // [n + 1] OUT ops per record (peek), then their exclusive prefix
    uint32_t *ops;           // OUT (16-byte aligned)
    uint64_t ops_cap;
    uint8_t *status;         // [n] OUT RB_BAM_*
    uint64_t *src;           // [n] scratch: where in data the record's words lie (in the record, or in its CG:B,I tag)
};
extern "C" hipError_t rb_launch_bam_peek(const rb_bam_params *p, hipStream_t stream);
extern "C" hipError_t rb_launch_bam_copy(const rb_bam_params *p, hipStream_t stream);
extern "C" uint32_t rb_bam_aux_row_step(void);
extern "C" uint32_t rb_bam_aux_row_max(void);
extern "C" uint32_t rb_bam_aux_wave_step(void);
extern "C" uint32_t rb_bam_copy_row_step(void);
extern "C" uint32_t rb_bam_copy_row_max(void);
extern "C" uint32_t rb_bam_copy_wave_step(void);

// ---- k_bamreads.hip: the per-read index nucfreq's host code needs, from the columns of rb_dev_bam_records ----
struct rb_bam_reads_params {
    uint64_t n;
    const uint8_t *data;     // the stream rb_dev_bam_records read
    const uint64_t *rec_off; // [n]
    const uint32_t *rec_len; // [n]
    const int32_t *tid;      // [n]
    const int64_t *pos;      // [n]
    const uint32_t *flag;    // [n]
    const uint64_t *op_off;  // [n + 1]
    const uint32_t *ops;     // 16-byte aligned, readable to the next multiple of 4 words behind the last op
    const uint8_t *status;   // [n] RB_BAM_*
    uint64_t *seq_off;       // [n] OUT
    uint64_t *start_key;     // [n] OUT
    uint64_t *end_key_pmax;  // [n] OUT the reads' own end keys (0: does not enter), then their inclusive prefix maximum
    unsigned long long *first_unsorted; // OUT, set to ~0 before the pass
    uint64_t *blk;           // scratch: the maxima of the scan's workgroups, level by level
};
extern "C" hipError_t rb_launch_bam_reads(const rb_bam_reads_params *p, hipStream_t stream);
extern "C" uint32_t rb_bam_reads_row_step(void);
extern "C" uint32_t rb_bam_reads_row_max(void);
extern "C" uint32_t rb_bam_reads_wave_step(void);
extern "C" uint32_t rb_bam_reads_scan_block(void);
extern "C" size_t rb_bam_reads_blk_count(uint64_t n);

// ---- k_rows_batch.hip: the hit rows of a clip call as a dense batch ----
struct rb_rows_batch_params {
    const uint32_t *ops;      // the source batch's packed ops (descriptor rows point into them)
    const uint64_t *op_off;   // used as a table of starts only
    const uint8_t *src_strand;
    const uint32_t *src_contig;
    const rb_hit_row *rows;
    uint64_t n_rows;
    const uint32_t *out_ops;
    uint64_t pieces_cap, ops_cap;
    uint64_t *cnt_ops;        // [n_rows + 1] scratch: ops per row, then their exclusive prefix
    uint64_t *cnt_pieces;     // [n_rows + 1] scratch: 1 per OK row, then the exclusive prefix (the row's piece)
    uint32_t *new_ops;
    uint64_t *new_op_off;
    uint64_t *t_st, *t_en, *q_st, *q_en;
    uint8_t *strand;
    uint32_t *contig, *parent;
    rb_pieces_info *info;
};
extern "C" hipError_t rb_launch_rows_batch_count(const rb_rows_batch_params *p, hipStream_t stream);
extern "C" hipError_t rb_launch_rows_batch_fill(const rb_rows_batch_params *p, hipStream_t stream);
extern "C" uint32_t rb_rtb_row_step(void);
extern "C" uint32_t rb_rtb_wave_step(void);
extern "C" uint32_t rb_rtb_row_max(void);

// ---- k_nucfreq.hip: nucfreq ----
struct rb_nf_params {
    uint64_t n_reads;
    const uint32_t *ops;
    const uint64_t *op_off;
    const uint8_t *seq;
    const uint64_t *seq_off;
    const uint32_t *l_seq;
    const int32_t *tid;
    const int64_t *pos;
    const uint32_t *flag;
    uint64_t n_regions;
    const int32_t *rg_tid;
    const uint64_t *rg_st, *rg_en, *out_off;
    uint32_t *counts;
    uint32_t *read_status;
    rb_nucfreq_counters *counters;
    // workspace
    uint64_t *end_key;  // [n_reads] tid << 32 | end, then its inclusive prefix maximum
    struct nf_read *hd; // [n_reads] what the tile kernel needs of a read, in one 48-byte record
    uint64_t *tile_off; // [n_regions + 1] exclusive prefix of tiles per region
    uint64_t *blk;      // block partials of the scans
    uint64_t *tile_lo, *tile_hi; // [max_tiles] reads that can overlap the tile
    uint64_t max_tiles;
    // htslib's cap on buffered reads (rb_k_nf_admit): per region the bit offset of its dropped-read bitmap in drop_bits (~0: none)
    uint64_t *drop_off;   // [n_regions]
    uint64_t *drop_bits;  // pool of drop_words 64-bit words; drop_bits[-1] is the pool's cursor
    uint64_t drop_words;
    uint32_t *deep_list;  // [n_regions + 1] regions whose fetch holds more reads than the cap; [n_regions] = how many
    uint32_t flags;       // bit 0: 16-bit counters for every tile (a diagnostic build of the tile kernel; the library passes 0)
    struct nf_tdesc *tdesc; // [max_tiles] what a workgroup needs to know about a tile, in one 64-byte record (rb_k_nf_tile_desc)
    uint32_t *wide_list;    // [max_tiles + 2] the tiles of the two builds that walk lists (rb_k_nf_tile_desc): [0] = how many of kind 2, then which,
                            // upwards from [1]; [max_tiles + 1] = how many of kind 0, then which, downwards from [max_tiles]
};
extern "C" hipError_t rb_launch_nucfreq(const rb_nf_params *p, hipStream_t stream);
extern "C" size_t rb_nf_tile_positions(void);
extern "C" size_t rb_nf_scan_blocks(uint64_t n);

// ---- k_nftext.hip: the lines of nucfreq ----
struct rb_nft_seg { // one segment as the kernel reads it (capi.hip packs the caller's seven arrays into these)
    uint64_t cnt;   // counts[4 * (cnt + k)] belongs to position pos + k
    uint32_t pos, n;
    uint32_t pre_off, suf_off, pre_len, suf_len;
};
struct rb_nft_params {
    const uint32_t *counts;   // 16-byte aligned
    uint64_t n_seg;
    const rb_nft_seg *seg;    // [n_seg]
    const uint32_t *unit0;    // [n_seg + 1] the first run of every segment; [n_seg] = n_units
    uint64_t n_units;         // runs of rb_nft_run() positions, all segments together
    const uint8_t *strings;
    int mode;                 // RB_NFT_FULL / RB_NFT_SMALL
    uint64_t *unit_off;       // [n_units + 1] bytes per run (sizes pass), then their exclusive prefix
    uint64_t *seg_text_off;   // [n_seg + 1] OUT
    uint64_t *seg_first;      // [n_seg] OUT, set to ~0 before the sizes pass
    uint64_t *seg_lines;      // [n_seg] OUT, zeroed before the sizes pass
    uint8_t *text;            // 16-byte aligned
    uint64_t text_cap;
};
extern "C" hipError_t rb_launch_nft(const rb_nft_params *p, bool fill, hipStream_t stream);
extern "C" hipError_t rb_launch_nft_seg_off(const rb_nft_params *p, hipStream_t stream);
extern "C" uint32_t rb_nft_step(void);
extern "C" uint32_t rb_nft_run(void);
extern "C" uint32_t rb_nft_block(void);
extern "C" uint32_t rb_nft_fix(void);

// ---- capi.hip: the library's own fill kernel (capi.hip says why) ----
extern "C" hipError_t rb_fill_async(void *dst, int value, size_t bytes, hipStream_t stream);
