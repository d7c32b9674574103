// rb_host.hpp -- C++ host mirror of the reference's interface for the CIGAR-walk path, over the C ABI
// (include/rustybam_amd.h).  Same names, argument meaning and error behaviour as the Rust functions it
// stands in for; where the reference panics this layer throws rb::Panic (the rb binary then exits 101,
// Rust's panic exit code).  Text decode/encode stays on the CPU; every CIGAR walk goes to the device.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <functional>
#include <string>
#include <vector>

#include "../../../include/rustybam_amd.h"

namespace rb {

struct Panic : std::runtime_error {
    using std::runtime_error::runtime_error;
};

// paf::PafRecord (paf.rs:346-368); cigar is packed len << 4 | op
struct PafRecord {
    std::string q_name;
    uint64_t q_len = 0, q_st = 0, q_en = 0;
    char strand = '+';
    std::string t_name;
    uint64_t t_len = 0, t_st = 0, t_en = 0, nmatch = 0, aln_len = 0, mapq = 0;
    std::vector<uint32_t> cigar;
    std::string id;
    uint64_t order = 0;            // set by Paf::orient (paf.rs:143)
    std::string to_string() const; // impl Display (paf.rs:923-944)
};

// bed::Region (bed.rs:15-21)
struct Region {
    std::string name;
    uint64_t st = 0, en = 0;
    std::string id;
};

// bamstats::Stats (bamstats.rs:16-36)
struct Stats {
    std::string q_nm, r_nm;
    int64_t q_len = 0, q_st = 0, q_en = 0, r_len = 0, r_st = 0, r_en = 0;
    char strand = '+';
    uint32_t equal = 0, diff = 0, ins = 0, del = 0, matches = 0, ins_events = 0, del_events = 0;
    float id_by_all = 0, id_by_events = 0, id_by_matches = 0;
    bool warn_m = false; // an alignment record with M and no MD tag: the reference warns when it gets to it (bamstats.rs:145-153)
};

class Engine { // one rb_ctx
  public:
    explicit Engine(int device = 0);
    ~Engine();
    rb_ctx *ctx() const { return ctx_; }
    int bsearch_policy = RB_BSEARCH_MODERN;
    void check(int rc, const char *what) const;

  private:
    rb_ctx *ctx_ = nullptr;
};

struct Paf { // paf::Paf (paf.rs:34-37)
    std::vector<PafRecord> records;
    // Paf::from_file (paf.rs:62-78): decode + check_integrity().unwrap() on every record (on the device)
    static Paf from_file(Engine &eng, const std::string &file_name);
    // Paf::overlapping_paf_recs (paf.rs:210-305)
    void overlapping_paf_recs(Engine &eng, int match_score, int diff_score, int indel_score, bool remove_contained);
    // header-only commands that sit between the CIGAR-walk stages of a pipeline (no device work: they never touch a CIGAR)
    void filter_aln_pairs(uint64_t paired_len);  // paf.rs:91-102
    void filter_query_len(uint64_t min_query_len); // paf.rs:104-106
    void filter_aln_len(uint64_t min_aln_len);   // paf.rs:109-111
    void orient();                               // paf.rs:114-157 (panics on a zero-bp (target, query) pair: divide by zero)
    void scaffold(uint64_t spacer_size);         // paf.rs:160-207
};

// `rb --gpus N` (the record shards of liftover.rs:123-129, one worker process per GPU): the readers below then load only bytes
// [begin, end) of a plain input file; read_input_text: the whole decompressed text of a file or stdin ("-")
void set_input_slice(uint64_t begin, uint64_t end);
// `rb --gpus N trim-paf` (query groups are the unit, paf.rs:223): the readers keep only the lines whose query name lies in [lo, hi)
// (bytewise order, nullptr = open); query_name_cuts: the names that cut a plain file's sorted query names into n ranges of about equal bytes
void set_input_query_range(const std::string *lo, const std::string *hi);
std::vector<std::string> query_name_cuts(const std::string &file_name, int n);
// where the contigs lie in a liftover output (canonical order is contig-major, liftover.rs:151-164): what `rb --gpus N` needs to
// put the shards' outputs together.  contigs = target names of the (possibly swapped) records in order of first appearance,
// runs = (index into contigs, bytes of output text) in output order
struct TextRuns {
    std::vector<std::string> contigs;
    std::vector<std::pair<uint32_t, uint64_t>> runs;
};
std::string read_input_text(const std::string &file_name);

std::string cigar_to_string(const std::vector<uint32_t> &cigar);
std::vector<std::string> records_to_text(const std::vector<PafRecord> &recs); // `println!("{}", rec)` for every record, encoded on all host cores; chunks in output order
// PafRecord::new (paf.rs:379-430): 0 = ok, 1 = Err(ParsePafColumn) (caller skips the line); throws Panic
int paf_record_new(const std::string &line, PafRecord &out);
std::vector<Region> parse_bed(const std::string &filename);                    // bed.rs:172-194
std::string f32_display(float v);                                              // Rust `{}` for f32

// paf_swap_query_and_target for a whole record set (paf.rs:1068-1094)
std::vector<PafRecord> paf_swap_query_and_target(Engine &eng, const std::vector<PafRecord> &recs);
// liftover::trim_paf_by_rgns (liftover.rs:134-167), single-thread output order
std::vector<PafRecord> trim_paf_by_rgns(Engine &eng, const std::vector<Region> &rgns, const std::vector<PafRecord> &paf_recs, bool invert_query);
// the same, printed: every Some(rec) as `println!("{}", rec)` would, without materialising the records
std::vector<std::string> trim_paf_by_rgns_text(Engine &eng, const std::vector<Region> &rgns, const std::vector<PafRecord> &paf_recs, bool invert_query,
                                               TextRuns *runs = nullptr);
// main.rs:186-214 without --largest, text in -> text out: the CIGAR text is parsed and printed on the device
// (rb_host_liftover_text); false = the file needs the general path (a line with two cg tags), nothing was produced.
// qbed (liftover.rs:139-148): the records are swapped first -- the parsed CIGARs in place on the device (RB_LIFT_QBED), the columns when
// the lines are put together; contigs (runs) are then the records' query names
bool liftover_file_text(Engine &eng, const std::string &paf_path, const std::vector<Region> &rgns, std::vector<std::string> &out_text,
                        TextRuns *runs = nullptr, bool qbed = false);
// main.rs:186-214 with --largest, text in -> text out: the hit rows never leave the device, rb_dev_largest keeps the last record of
// largest target span per id (main.rs:200-208) and only those records are printed, in id order (rb_host_liftover_largest_text); false = take
// the record route (two cg tags, a stripped record that lies inside a window, a hit row that panics), nothing was produced
bool liftover_largest_file_text(Engine &eng, const std::string &paf_path, const std::vector<Region> &rgns, std::vector<std::string> &out_text,
                                bool qbed = false);
// `rb liftover --stats` / `rb break-paf --stats` (this project's own flags): the lines `rb liftover .. | rb stats --paf [--qbed]` prints,
// without the header -- one cigar_stats_line per record the plain command prints, from rb_dev_stats_rows of the clips where they lie; no
// CIGAR text is printed or parsed in between.  The *_file_text forms: text in, rb_host_liftover_stats_text / rb_host_break_stats_text;
// false = take the record route (the *_stats_text forms below), nothing was produced.  A panic of the plain command is thrown.
// trailing_panic: the message of the second command's panic on a record the first printed (never, for clips the kernels wrote): the
// lines in front of it are returned
bool liftover_stats_file_text(Engine &eng, const std::string &paf_path, const std::vector<Region> &rgns, bool qbed, bool stats_qbed,
                              std::vector<std::string> &out_text, std::string &trailing_panic);
bool break_stats_file_text(Engine &eng, const std::string &paf_path, uint32_t break_length, bool stats_qbed, std::vector<std::string> &out_text,
                           std::string &trailing_panic);
std::vector<std::string> trim_paf_by_rgns_stats_text(Engine &eng, const std::vector<Region> &rgns, const std::vector<PafRecord> &paf_recs, bool invert_query,
                                                     bool stats_qbed, std::string &trailing_panic);
std::vector<std::string> break_paf_on_indels_stats_text(Engine &eng, const std::vector<PafRecord> &paf_recs, uint32_t break_length, bool stats_qbed,
                                                        std::string &trailing_panic);
// `rb liftover --bed W --break N [--stats | --stats-qbed]` (this project's own flag): what `rb break-paf --max-size N in.paf | rb liftover
// --bed W -` prints (with stats_mode 1 / 2: what `| rb stats --paf [--qbed] -` behind it prints, without the header), the pieces never
// printed or read back.  The second command sees the printed pieces: their own id is empty again, contigs are ordered by first appearance
// among the pieces, names, lengths and mapq are the parent record's.
//   break_liftover_file_text   text in, rb_host_break_liftover_text / _stats_text; false = take the record route, nothing was produced
//   break_liftover_[stats_]text the record route: break_paf_on_indels, the pieces re-read, trim_paf_by_rgns.  first_panic: the first command
//                              panicked part-way (main.rs:274-280 prints record by record): what the second command makes of the pieces
//                              printed by then is returned, the message goes here.  A panic of the second command is thrown.
bool break_liftover_file_text(Engine &eng, const std::string &paf_path, const std::vector<Region> &rgns, uint32_t break_length, int stats_mode,
                              std::vector<std::string> &out_text, std::string &trailing_panic);
std::vector<std::string> break_liftover_text(Engine &eng, const std::vector<Region> &rgns, const std::vector<PafRecord> &paf_recs, uint32_t break_length,
                                             std::string &first_panic);
std::vector<std::string> break_liftover_stats_text(Engine &eng, const std::vector<Region> &rgns, const std::vector<PafRecord> &paf_recs, uint32_t break_length,
                                                   bool stats_qbed, std::string &first_panic, std::string &trailing_panic);
// `rb break-paf --max-size N [--orient] [--paired-len L] [--aln A] [--query Q] [--stats | --stats-qbed]` (this project's own flags): what
// `rb break-paf --max-size N in.paf [| rb orient -] [| rb filter --paired-len L --aln A --query Q -] [| rb stats --paf [--qbed] -]` prints
// (stats_mode 1 / 2: without the header), the pieces never printed or read back.  Orient and filter are sums over the pieces' headers keyed by
// the (target name, query name) pair: rb_dev_pairs_rows on the hit rows of rb_dev_break.
//   break_pairs_file_text  text in, rb_host_break_pairs_text / _stats_text; false = take the record route, nothing was produced
//   break_pairs_text       the record route: break_paf_on_indels, the pieces re-read with an empty id, Paf::orient, Paf::filter_*, then
//                          records_to_text or stats_from_paf.  first_panic as in break_liftover_text; a later command's panic is thrown.
bool break_pairs_file_text(Engine &eng, const std::string &paf_path, uint32_t break_length, bool orient, bool filter, uint64_t paired_len, uint64_t min_aln,
                           uint64_t min_query, int stats_mode, std::vector<std::string> &out_text, std::string &trailing_panic);
std::vector<std::string> break_pairs_text(Engine &eng, const std::vector<PafRecord> &paf_recs, uint32_t break_length, bool orient, bool filter,
                                          uint64_t paired_len, uint64_t min_aln, uint64_t min_query, int stats_mode, std::string &first_panic);
// `rb orient [--scaffold --insert I]` / `rb filter -p L -a A -q Q` (main.rs:234-267), text in -> text out for a file or stdin
// (rb_host_pairs_text: rb_dev_pairs_records on the records, the kept records' CIGARs printed on the device; --scaffold sorts an index array
// on the host); false = take the record route (Paf::from_file, Paf::orient / scaffold / filter_*, records_to_text), nothing was produced
bool orient_file_text(Engine &eng, const std::string &paf_path, bool scaffold, uint64_t spacer, std::vector<std::string> &out_text);
bool filter_file_text(Engine &eng, const std::string &paf_path, uint64_t paired_len, uint64_t min_aln, uint64_t min_query, std::vector<std::string> &out_text);
// the same two routes as a pipeline over chunks of a big plain file (a few host threads, each with its own context on `device`):
// the sink receives the chunks' outputs in file order while later chunks are still being read / clipped / printed.  A chunk's text
// is contig-major within the chunk (runs); false = not applicable or a line needs the general parser (pipeline_started(): the
// sink has already been given chunks)
bool lift_file_text_pipelined(int device, int bsearch_policy, bool is_break, uint32_t break_length, const std::string &paf_path,
                              const std::vector<Region> &rgns, const std::function<bool(std::vector<std::string> &, TextRuns &)> &sink); // sink: false = stop, the caller takes the whole-file route
bool pipeline_started();
bool break_file_text(Engine &eng, const std::string &paf_path, uint32_t break_length, std::vector<std::string> &out_text); // main.rs:271-281
bool trim_file_text(Engine &eng, const std::string &paf_path, int match_score, int diff_score, int indel_score, bool remove_contained,
                    std::vector<std::string> &out_text); // main.rs:218-230, the batch resident on the device across the passes
bool invert_file_text(Engine &eng, const std::string &paf_path, std::vector<std::string> &out_text); // main.rs:176-182, CIGARs parsed, swapped and printed on the device
bool stats_file_text(Engine &eng, const std::string &paf_path, bool qbed, std::vector<std::string> &out_text);          // main.rs:50-58, lines without the header
std::vector<std::string> break_paf_on_indels_text(Engine &eng, const std::vector<PafRecord> &paf_recs, uint32_t break_length);
// main.rs:274-280: aligned_pairs + liftover::break_paf_on_indels (liftover.rs:182-226) for every record, record order
std::vector<PafRecord> break_paf_on_indels(Engine &eng, const std::vector<PafRecord> &paf_recs, uint32_t break_length);
// bamstats::stats_from_paf (bamstats.rs:91-154) for every record
std::vector<Stats> stats_from_paf(Engine &eng, const std::vector<PafRecord> &paf_recs);
// bamstats::parse_md_for_stats (bamstats.rs:48-79): (match_count, mismatch_count, insertion_count, insertion_bases)
void parse_md_for_stats(const std::string &md, uint32_t out[4]);
// main.rs:60-77 + bamstats::cigar_stats (bamstats.rs:156-222): every mapped record of a BAM file (BGZF through zlib);
// the CIGAR counters come from the device record-scan kernel (BAM cigars are already the packed u32 form)
// trailing_panic: where the reference panics part-way through the file (a broken record, read_pos), the stats of the records
// before it come back and the panic message goes here (NULL: thrown instead) -- the reference has printed them by then
std::vector<Stats> cigar_stats_bam(Engine &eng, const std::string &bam_path, std::string *trailing_panic = nullptr);
// `rb stats <in>` without --paf reads "sam/bam/cram" in the reference (cli.rs:49-60).  stats_input_kind looks at the first four
// (decompressed) bytes of the file, or of stdin -- which is read once and kept --: BAM\1, CRAM, or text.
// stats_sam_text: SAM text in, stats lines out (chunks in output order, without the header) on the device: the text uploaded once,
// rb_dev_parse_cigars on the CIGAR columns, rb_dev_scan_records, rb_dev_parse_md on the MD:Z: values of every record that has one,
// rb_dev_aln_stats, the rows back, the lines assembled on all host cores.  stats_sam_records: the record route (RB_GENERAL_PATH=1):
// CIGAR text parsed on the host, rb_host_scan_records, the host's parse_md_for_stats.  Both: false = the text is not SAM (its first
// byte is not '@' and its first line has fewer than 11 columns), nothing was produced.  The lines of the records in front of the first
// one the reference dies on come back, its panic in trailing_panic (empty: none).  RB_TIMING=1: stats_sam_text names itself, its laps
// and how many records it left to the host (a CIGAR or MD number of ten or more digits) on stderr.
enum { STATS_INPUT_BAM = 0, STATS_INPUT_TEXT = 1, STATS_INPUT_CRAM = 2 };
int stats_input_kind(const std::string &path);
bool stats_sam_text(Engine &eng, const std::string &path, bool qbed, std::vector<std::string> &out_text, std::string &trailing_panic);
bool stats_sam_records(Engine &eng, const std::string &path, bool qbed, std::vector<std::string> &out_text, std::string &trailing_panic);
// stats_bam_text: BAM in (a file or stdin, BGZF or plain gzip), stats lines out on the device: the stream inflated as cigar_stats_bam
// does, the records hopped through on the host (one read each, and the two truncation panics), the stream uploaded once,
// rb_dev_bam_records (fields, MD:Z and CG:B,I of the aux area, the CIGAR words gathered into aligned ops), rb_dev_scan_records,
// rb_dev_parse_md on the MD values where they lie in the stream, rb_dev_aln_stats, the rows back, the lines assembled on all host cores
// (query names from the host's copy, reference names from the header).  The lines of the mapped records in front of the first record the
// reference dies on come back, its panic in trailing_panic.  A header that is broken throws, as cigar_stats_bam does.  RB_TIMING=1:
// names itself, its laps and how many records it left to the host (an MD number of ten or more digits).
void stats_bam_text(Engine &eng, const std::string &path, bool qbed, std::vector<std::string> &out_text, std::string &trailing_panic);
std::string cigar_stats_header(bool qbed);              // bamstats.rs:225-236
// bed::parse_region (bed.rs:88-131): "name:st-en", 1-based inclusive start -> 0-based half-open; id = the same text
Region parse_region(const std::string &region);
// main.rs:82-121 + nucfreq.rs: A/C/G/T counts at every covered position of every region, printed piece by piece (1 Mbp) through
// `put`; BGZF/BAM decode on the host, the pileup and the lines on the device (rb_host_nucfreq_text: the counts stay there, the text of
// a piece comes back and goes out through `put_bytes` behind the header line the host writes through `put`) -- by default for --small,
// with RB_NUCFREQ_TEXT=1 for the full format too (profiles/nucfreq_text_summary.md says why not by default).  RB_GENERAL_PATH=1, and a
// region whose name + TAB or TAB + id + LF is longer than the kernel's 255 bytes: rb_host_nucfreq, the counts back, the lines formatted on
// all host cores.  So does, on either route, a batch of regions that no read reaches: nothing is sent to the device for it, and it prints
// header lines only.  RB_TIMING=1: the text route names itself ("[rb timing] nucfreq_text: ...") the first time a batch takes it, and a
// batch on it has one lap ("nucfreq: device + lines + write") where the host formatter has two ("nucfreq: device", "nucfreq: format + write").
void nucfreq_bam(Engine &eng, const std::string &bam_path, const std::vector<Region> &rgns, bool small,
                 const std::function<void(const std::string &)> &put, const std::function<void(const char *, size_t)> &put_bytes);
std::string cigar_stats_line(const Stats &s, bool qbed); // bamstats.rs:239-270

} // namespace rb
