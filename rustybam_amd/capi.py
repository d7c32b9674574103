"""ctypes binding of include/rustybam_amd.h (plumbing for tests and bench.py)."""
import ctypes as C
import os
import sys
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "rustybam_amd.h")

BSEARCH_MODERN, BSEARCH_LEGACY, LIFT_EARLY_EXIT, LIFT_DESCRIPTORS, LIFT_FUSED_SCAN = 0, 1, 16, 32, 64
TRIM_IN_PLACE = 256  # rb_dev_overlap_split on a resident batch (out_ops = the batch's ops): regular records are cut where they are, not copied
LIFT_OP_STARTS = 1 << 20  # rb_dev_liftover / rb_dev_break on a batch trim-paf has cut in place: op_off is a table of starts, extents come from the norm rows
BREAK_ONE_WALK = 128  # rb_dev_break: the clip kernel finds the long indels itself; records it declines are done in the same call
HIT_INSIDE, HIT_GENERIC, HIT_DESCRIPTOR = 1, 2, 4
NF_COVERED = 0x80000000
RD_OK, RD_FILTERED, RD_BAD_CIGAR, RD_SEQ_SHORT = 0, 1, 2, 3
NFT_FULL, NFT_SMALL = 0, 1  # rb_dev_nucfreq_text modes

REDUCE_DT = np.dtype(
    [("t_bases", "<u8"), ("q_bases", "<u8"), ("nmatch", "<u4"), ("aln_len", "<u4"), ("equal", "<u4"),
     ("diff", "<u4"), ("ins", "<u4"), ("del", "<u4"), ("matches", "<u4"), ("ins_events", "<u4"),
     ("del_events", "<u4"), ("id_by_all", "<f4"), ("id_by_events", "<f4"), ("id_by_matches", "<f4"),
     ("status", "<u4"), ("flags", "<u4")])
NORM_DT = np.dtype(
    [("t_st", "<u8"), ("t_en", "<u8"), ("q_st", "<u8"), ("q_en", "<u8"), ("first_op", "<u4"), ("n_ops", "<u4"),
     ("lead_ops", "<u4"), ("trail_ops", "<u4"), ("nmatch", "<u4"), ("aln_len", "<u4"), ("status", "<u4"),
     ("flags", "<u4")])
HIT_DT = np.dtype(
    [("rec", "<u4"), ("win", "<u4"), ("status", "<u2"), ("flags", "<u2"), ("out_n", "<u4"), ("t_st", "<u8"),
     ("t_en", "<u8"), ("q_st", "<u8"), ("q_en", "<u8"), ("nmatch", "<u4"), ("aln_len", "<u4"), ("out_off", "<u8")])
PAIR_DT = np.dtype(
    [("split_idx", "<u8"), ("split_score", "<i4"), ("status", "<u4"), ("t_st", "<u8", 2), ("t_en", "<u8", 2),
     ("q_st", "<u8", 2), ("q_en", "<u8", 2), ("nmatch", "<u4", 2), ("aln_len", "<u4", 2), ("out_off", "<u8", 2),
     ("out_n", "<u4", 2), ("_pad", "<u4"), ("_row", "<u4")])  # (the diagnostic word's halves: _pad 1 = cut by a wave kernel, _row 1 = by the row kernel)
TRIM_PASS_DT = np.dtype([("n_pairs", "<u8"), ("n_deferred", "<u8"), ("ops_end", "<u8"), ("bad_status", "<u4"), ("_pad", "<u4"), ("_reserved", "<u8", 4)])
COUNTERS_DT = np.dtype(
    [("n_hits", "<u8"), ("out_ops_needed", "<u8"), ("out_ops_used", "<u8"), ("n_generic", "<u8"),
     ("overflow", "<u4"), ("phase", "<u4", 5), ("brk_scratch_short", "<u4"), ("redo_two_walk", "<u4")])
assert REDUCE_DT.itemsize == 72 and NORM_DT.itemsize == 64 and HIT_DT.itemsize == 64 and COUNTERS_DT.itemsize == 64
assert PAIR_DT.itemsize == 128
PIECES_INFO_DT = np.dtype([("n_pieces", "<u8"), ("n_ops", "<u8"), ("overflow", "<u4"), ("declined", "<u4"), ("_reserved", "<u8", 5)])  # rb_pieces_info
assert PIECES_INFO_DT.itemsize == 64
PAIRS_INFO_DT = np.dtype([("n_kept", "<u8"), ("n_flipped_rows", "<u8"), ("overflow", "<u4"), ("declined", "<u4"), ("_reserved", "<u8", 5)])  # rb_pairs_info
assert PAIRS_INFO_DT.itemsize == 64
PAIRS_ORIENT, PAIRS_FILTER = 1, 2  # rb_dev_pairs_rows: mode
ALN_DT = np.dtype(
    [("r_en", "<i8"), ("q_st", "<i8"), ("q_en", "<i8"), ("q_len", "<i8"), ("equal", "<u4"), ("diff", "<u4"), ("ins", "<u4"), ("del", "<u4"),
     ("matches", "<u4"), ("ins_events", "<u4"), ("del_events", "<u4"), ("id_by_all", "<f4"), ("id_by_events", "<f4"), ("id_by_matches", "<f4"),
     ("status", "<u4"), ("flags", "<u4")])  # rb_aln_row
assert ALN_DT.itemsize == 80
MD_OK, MD_UNUSUAL = 0, 3  # rb_dev_parse_md: status
ALN_OK, ALN_PANIC_DEL_FIRST, ALN_PANIC_HARDCLIP, ALN_PANIC_NONE, ALN_PANIC_MD_ASSERT, ALN_MD_STATUS = 0, 32, 33, 34, 35, 64  # rb_aln_row.status
ALN_WARN_M = 1  # rb_aln_row.flags
BAM_OK, BAM_SHORT_BLOCK, BAM_NO_FIT, BAM_BAD_NAME = 0, 1, 2, 3  # rb_dev_bam_records: status
PAIRS_DECL_PANIC, PAIRS_DECL_KEY, PAIRS_DECL_WRAP, PAIRS_DECL_ZERO_SPAN = 1, 2, 4, 8  # rb_pairs_info.declined


def hit_rows_from(rows):
    """Rows of another layout with the same field names (the oracle's 72-byte rows) as rb_hit_row records (HIT_DT, 64 bytes): what
    rb_dev_digest_rows reads.  flags keeps bit 0 only (HIT_INSIDE)."""
    out = np.zeros(len(rows), dtype=HIT_DT)
    for k in ("rec", "win", "out_n", "t_st", "t_en", "q_st", "q_en", "nmatch", "aln_len", "out_off"):
        out[k] = rows[k]
    out["status"] = rows["status"].astype(np.uint16)
    out["flags"] = (rows["flags"] & 1).astype(np.uint16)
    return out


class RbError(RuntimeError):
    pass


def lib_path():
    """the product library; RB_VARIANT=<name> (diagnostics only: tools/mkvariant.sh builds rustybam_amd/variants/<name>.so, some of them
    timing builds with wrong results) loads that one instead and says so -- the A/B scripts select a variant this way and never copy
    one over the product library"""
    v = os.environ.get("RB_VARIANT")
    if v:
        p = os.path.join(HERE, "variants", v + ".so")
        print(f"[rustybam_amd] RB_VARIANT: loading {p} instead of the product library", file=sys.stderr)
        return p
    return os.path.join(HERE, "librustybam_amd.so")


_lib = None


def lib():
    """Load the product library.  Raises if it has not been built (no CPU fallback exists)."""
    global _lib
    if _lib is None:
        p = lib_path()
        if not os.path.exists(p):
            raise RbError(f"{p} is missing: run `make -C rustybam_amd/csrc` (or __graft_entry__.build())")
        _lib = C.CDLL(p)
        _lib.rb_ctx_last_error.restype = C.c_char_p
        _lib.rb_ctx_stream.restype = C.c_void_p
        _lib.rb_plan_workspace_bytes.restype = C.c_size_t
        _lib.rb_plan_diag_stamps_offset.restype = C.c_size_t
        _lib.rb_plan_out_capacity.restype = C.c_uint64
        _lib.rb_synth_n_ops.restype = C.c_uint32
        _lib.rb_synth_n_ops.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32]
    return _lib


def declared_symbols():
    """Every function name declared in include/rustybam_amd.h."""
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(rb_[a-z0-9_]+)\s*\(", txt)))


def exported_symbols():
    out = []
    L = lib()
    for s in declared_symbols():
        try:
            getattr(L, s)
            out.append(s)
        except AttributeError:
            pass
    return out


def rows_to_batch_shape():
    """(ops per step of a row of 16 lanes, longest clip a row takes, ops per step of the wavefront) of rb_dev_rows_to_batch's copy kernel
    (rb_rows_to_batch_shape: no device needed)"""
    out = (C.c_uint32 * 3)()
    f = lib().rb_rows_to_batch_shape
    f.restype = None
    f(out)
    return tuple(int(x) for x in out)


def nucfreq_text_shape():
    """(positions per wavefront step, positions per workgroup, longest prefix, longest suffix) of rb_dev_nucfreq_text's kernel
    (rb_nucfreq_text_shape: no device needed)"""
    out = (C.c_uint32 * 4)()
    f = lib().rb_nucfreq_text_shape
    f.restype = None
    f(out)
    return tuple(int(x) for x in out)


def md_shape():
    """(bytes per step of a row of 16 lanes, longest string a row takes, bytes per step of the wavefront) of rb_dev_parse_md's kernel
    (rb_md_shape: no device needed)"""
    out = (C.c_uint32 * 3)()
    f = lib().rb_md_shape
    f.restype = None
    f(out)
    return tuple(int(x) for x in out)


def bam_shape():
    """rb_dev_bam_records' kernels (rb_bam_shape: no device needed): (bytes per step of a row of 16 lanes in the search for a NUL, longest
    aux area a row walks, bytes per step of the wavefront; ops per step of a row in the copy, longest CIGAR a row copies, ops per step
    of the wavefront)"""
    out = (C.c_uint32 * 6)()
    f = lib().rb_bam_shape
    f.restype = None
    f(out)
    return tuple(int(x) for x in out)


def bam_reads_shape():
    """rb_dev_bam_reads' kernels (rb_bam_reads_shape: no device needed): (ops per step of a row of 16 lanes, longest CIGAR a row sums, ops per
    step of the wavefront, records per workgroup of the scan)"""
    out = (C.c_uint32 * 4)()
    f = lib().rb_bam_reads_shape
    f.restype = None
    f(out)
    return tuple(int(x) for x in out)


def pairs_shape():
    """(consecutive rows one wavefront of rb_dev_pairs_rows' sum kernel walks, rows per workgroup) (rb_pairs_shape: no device needed)"""
    out = (C.c_uint32 * 2)()
    f = lib().rb_pairs_shape
    f.restype = None
    f(out)
    return tuple(int(x) for x in out)


def host_pairs_rows(rows, rec_key, rec_q_len, strand, n_keys, mode, paired_len=0, min_aln=0, min_query=0, rows_cap=None):
    """rb_host_pairs_rows: orient / filter over hit rows in plain C++ on host arrays (no device, no context)
    -> (rows_out HIT_DT [min(n_kept, rows_cap)], key_flip u8 [n_keys], info PAIRS_INFO_DT)"""
    rows, rec_key = _arr(rows, HIT_DT), _arr(rec_key, np.uint32)
    rec_q_len, strand = _arr(rec_q_len, np.uint64), _arr(strand, np.uint8)
    cap = len(rows) if rows_cap is None else int(rows_cap)
    out, flip, info = np.zeros(cap, HIT_DT), np.zeros(int(n_keys), np.uint8), np.zeros(1, PAIRS_INFO_DT)
    rc = lib().rb_host_pairs_rows(_p(rows), C.c_uint64(len(rows)), _p(rec_key), _p(rec_q_len), _p(strand), C.c_uint64(len(rec_key)), C.c_uint64(int(n_keys)),
                                  C.c_uint32(mode), C.c_uint64(paired_len), C.c_uint64(min_aln), C.c_uint64(min_query), _p(out), C.c_uint64(cap), _p(flip),
                                  _p(info))
    if rc != 0:
        raise RbError(f"rb_host_pairs_rows failed with {rc}")
    return out[:min(int(info[0]["n_kept"]), cap)], flip, info[0]


def pairs_records_shape():
    """(consecutive records one wavefront of rb_dev_pairs_records' sum kernel walks, records per workgroup) (rb_pairs_records_shape: no device needed)"""
    out = (C.c_uint32 * 2)()
    f = lib().rb_pairs_records_shape
    f.restype = None
    f(out)
    return tuple(int(x) for x in out)


def _pairs_records_cols(t_st, t_en, q_st, q_en, strand, rec_key, rec_q_len):
    cols = [_arr(x, np.uint64) for x in (t_st, t_en, q_st, q_en)] + [_arr(strand, np.uint8), _arr(rec_key, np.uint32), _arr(rec_q_len, np.uint64)]
    assert len({len(c) for c in cols}) == 1, "the seven columns have one length"
    return cols


def host_pairs_records(t_st, t_en, q_st, q_en, strand, rec_key, rec_q_len, n_keys, mode, paired_len=0, min_aln=0, min_query=0, kept_cap=None):
    """rb_host_pairs_records: orient / filter over the records of a batch in plain C++ on host arrays (no device, no context)
    -> dict(kept u32 [min(n_kept, kept_cap)], q_st, q_en u64 [n_rec], key_flip u8 [n_keys], key_order u64 [n_keys], info PAIRS_INFO_DT)"""
    cols = _pairs_records_cols(t_st, t_en, q_st, q_en, strand, rec_key, rec_q_len)
    n, n_keys = len(cols[0]), int(n_keys)
    cap = n if kept_cap is None else int(kept_cap)
    kept, qs, qe = np.zeros(cap, np.uint32), np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    flip, order, info = np.zeros(n_keys, np.uint8), np.zeros(n_keys, np.uint64), np.zeros(1, PAIRS_INFO_DT)
    rc = lib().rb_host_pairs_records(*map(_p, cols), C.c_uint64(n), C.c_uint64(n_keys), C.c_uint32(mode), C.c_uint64(paired_len), C.c_uint64(min_aln),
                                     C.c_uint64(min_query), _p(kept) if cap else None, C.c_uint64(cap), _p(qs), _p(qe), _p(flip), _p(order), _p(info))
    if rc != 0:
        raise RbError(f"rb_host_pairs_records failed with {rc}")
    return dict(kept=kept[:min(int(info[0]["n_kept"]), cap)], q_st=qs, q_en=qe, key_flip=flip, key_order=order, info=info[0])


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None else C.c_void_p(0)


def _arr(x, dt):
    return np.ascontiguousarray(x, dtype=dt)


class ReadsView(C.Structure):
    """rb_reads_view"""
    _fields_ = [("n_reads", C.c_uint64), ("ops", C.c_void_p), ("op_off", C.c_void_p), ("seq", C.c_void_p), ("seq_off", C.c_void_p),
                ("l_seq", C.c_void_p), ("tid", C.c_void_p), ("pos", C.c_void_p), ("flag", C.c_void_p)]


class BatchView(C.Structure):
    _fields_ = [("n_rec", C.c_uint64), ("n_ops", C.c_uint64), ("ops", C.c_void_p), ("op_off", C.c_void_p),
                ("t_st", C.c_void_p), ("t_en", C.c_void_p), ("q_st", C.c_void_p), ("q_en", C.c_void_p),
                ("strand", C.c_void_p), ("contig", C.c_void_p)]


class Engine:
    """One rb_ctx.  `stream` is a raw hipStream_t (e.g. torch.cuda.current_stream().cuda_stream) or None."""

    def __init__(self, device=0, stream=None):
        self.L = lib()
        self.ctx = C.c_void_p()
        rc = self.L.rb_ctx_create(C.c_int(device), C.c_void_p(stream or 0), C.byref(self.ctx))
        if rc != 0:
            raise RbError(f"rb_ctx_create(device={device}) failed with {rc}: no usable gfx950 device "
                          f"(there is no CPU fallback)")

    def close(self):
        if self.ctx:
            self.L.rb_ctx_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != 0:
            raise RbError(f"{what} failed with {rc}: {self.L.rb_ctx_last_error(self.ctx).decode()}")

    def sync(self):
        self._chk(self.L.rb_ctx_sync(self.ctx), "rb_ctx_sync")

    # ---- device-pointer level (bench.py: buffers are torch tensors already resident in HBM) ----
    def trim_reserve(self, n_pairs):
        self._chk(self.L.rb_dev_trim_reserve(self.ctx, C.c_uint64(int(n_pairs))), "rb_dev_trim_reserve")

    def set_timing(self, on=True):
        self._chk(self.L.rb_ctx_set_timing(self.ctx, C.c_int(1 if on else 0)), "rb_ctx_set_timing")

    def get_timing(self):
        buf = (C.c_double * 256)()
        n = C.c_int()
        self._chk(self.L.rb_ctx_get_timing(self.ctx, buf, C.c_int(256), C.byref(n)), "rb_ctx_get_timing")
        return [buf[i] for i in range(n.value)]

    @staticmethod
    def batch_view(n_rec, n_ops, ops, op_off, t_st, t_en, q_st, q_en, strand, contig):
        """All arguments after n_ops are raw device addresses (ints)."""
        return BatchView(n_rec, n_ops, ops, op_off, t_st, t_en, q_st, q_en, strand, contig)

    def dev_synth_fill_ops(self, seed, first_record, n_rec, op_off_ptr, ops_ptr):
        self._chk(self.L.rb_dev_synth_fill_ops(self.ctx, C.c_uint64(seed), C.c_uint64(first_record), C.c_uint64(n_rec),
                                               C.c_void_p(op_off_ptr), C.c_void_p(ops_ptr)), "rb_dev_synth_fill_ops")

    def dev_scan_records(self, view, reduce_ptr, norm_ptr):
        self._chk(self.L.rb_dev_scan_records(self.ctx, C.byref(view), C.c_void_p(reduce_ptr or 0),
                                             C.c_void_p(norm_ptr or 0)), "rb_dev_scan_records")

    def scan_route(self):
        """-> (records the row form of the last scan on this context took itself, records it listed for the wave-per-record kernel);
        (0, 0): the wave-per-record kernel took the whole batch (rb_ctx_scan_route)"""
        o = (C.c_uint64 * 2)()
        self._chk(self.L.rb_ctx_scan_route(self.ctx, o), "rb_ctx_scan_route")
        return int(o[0]), int(o[1])

    def dev_digest_rows(self, view, rows_ptr, n_rows, out_ptr, row_base, rec_base, digest_ptr):
        self._chk(self.L.rb_dev_digest_rows(self.ctx, C.byref(view), C.c_void_p(rows_ptr), C.c_uint64(n_rows), C.c_void_p(out_ptr),
                                            C.c_uint64(row_base), C.c_uint64(rec_base), C.c_void_p(digest_ptr)), "rb_dev_digest_rows")

    def dev_overlap_split(self, view, norm_ptr, n_pairs, left_ptr, right_ptr, pair_out_off_ptr, scores, policy, rows_ptr, out_ptr):
        self._chk(self.L.rb_dev_overlap_split(self.ctx, C.byref(view), C.c_void_p(norm_ptr), C.c_uint64(n_pairs), C.c_void_p(left_ptr),
                                              C.c_void_p(right_ptr), C.c_void_p(pair_out_off_ptr), C.c_int(scores[0]), C.c_int(scores[1]),
                                              C.c_int(scores[2]), C.c_int(policy), C.c_void_p(rows_ptr), C.c_void_p(out_ptr)), "rb_dev_overlap_split")

    def dev_apply_pairs(self, n_pairs, left_ptr, right_ptr, rows_ptr, op_off_ptr, norm_ptr):
        self._chk(self.L.rb_dev_apply_pairs(self.ctx, C.c_uint64(n_pairs), C.c_void_p(left_ptr), C.c_void_p(right_ptr), C.c_void_p(rows_ptr),
                                            C.c_void_p(op_off_ptr), C.c_void_p(norm_ptr)), "rb_dev_apply_pairs")

    def trim_select_scratch_bytes(self, n_groups):
        f = self.L.rb_trim_select_scratch_bytes
        f.restype = C.c_size_t
        return int(f(C.c_uint64(n_groups)))

    def dev_trim_select(self, n_rec, n_groups, order_ptr, grp_off_ptr, norm_ptr, out_base, contained_ptr, left_ptr, right_ptr, pair_out_off_ptr,
                        pass_ptr, scratch_ptr):
        self._chk(self.L.rb_dev_trim_select(self.ctx, C.c_uint64(n_rec), C.c_uint64(n_groups), C.c_void_p(order_ptr), C.c_void_p(grp_off_ptr),
                                            C.c_void_p(norm_ptr), C.c_uint64(out_base), C.c_void_p(contained_ptr), C.c_void_p(left_ptr),
                                            C.c_void_p(right_ptr), C.c_void_p(pair_out_off_ptr), C.c_void_p(pass_ptr), C.c_void_p(scratch_ptr)),
                  "rb_dev_trim_select")

    def dev_trim_check(self, n_pairs, rows_ptr, pass_ptr):
        self._chk(self.L.rb_dev_trim_check(self.ctx, C.c_uint64(n_pairs), C.c_void_p(rows_ptr), C.c_void_p(pass_ptr)), "rb_dev_trim_check")

    def dev_gather_records(self, n_rec, ops_ptr, op_off_ptr, norm_ptr, new_off_ptr, new_ops_ptr, scratch_ptr):
        self._chk(self.L.rb_dev_gather_records(self.ctx, C.c_uint64(n_rec), C.c_void_p(ops_ptr), C.c_void_p(op_off_ptr), C.c_void_p(norm_ptr),
                                               C.c_void_p(new_off_ptr), C.c_void_p(new_ops_ptr or 0), C.c_void_p(scratch_ptr)), "rb_dev_gather_records")

    def dev_alloc(self, n_bytes):
        """device memory from the library's allocator (requests of 256 MB and more: 2 MB physical chunks mapped side by side); -> address"""
        d = C.c_void_p()
        self._chk(self.L.rb_dev_alloc(self.ctx, C.c_size_t(n_bytes), C.byref(d)), "rb_dev_alloc")
        return int(d.value)

    SCORE_CB = C.CFUNCTYPE(C.c_double, C.c_void_p, C.c_void_p)

    def dev_alloc_placed(self, n_bytes, tries, score=None):
        """a buffer that will be written at streaming rate, placed by measurement (rb_dev_alloc_placed: up to `tries` candidates, a store
        sweep over each -- or score(address) -> time, the caller's own launch (rb_dev_alloc_placed_by) --, the fastest kept);
        -> (address, [score per candidate], index kept)"""
        d, kept = C.c_void_p(), C.c_int(-1)
        ms = (C.c_double * max(1, tries))()
        if score is None:
            self._chk(self.L.rb_dev_alloc_placed(self.ctx, C.c_uint64(n_bytes), C.c_int(tries), C.byref(d), ms, C.byref(kept)), "rb_dev_alloc_placed")
        else:
            err = []

            def cb(ptr, _user):
                try:
                    return float(score(int(ptr)))
                except Exception as e:  # (no exception may cross the C frames: the search ends, the caller hears about it below)
                    err.append(e)
                    return -1.0
            fn = self.SCORE_CB(cb)
            rc = self.L.rb_dev_alloc_placed_by(self.ctx, C.c_uint64(n_bytes), C.c_int(tries), fn, None, C.byref(d), ms, C.byref(kept))
            if err:
                raise err[0]
            self._chk(rc, "rb_dev_alloc_placed_by")
        return int(d.value), [round(ms[i], 4) for i in range(tries) if ms[i] >= 0], int(kept.value)

    def dev_free(self, ptr):
        self._chk(self.L.rb_dev_free(self.ctx, C.c_void_p(ptr)), "rb_dev_free")

    def dev_release(self, ptr):
        """back to the context's cache: still mapped, handed out again by the next dev_alloc / dev_alloc_placed of the same size"""
        self._chk(self.L.rb_dev_release(self.ctx, C.c_void_p(ptr)), "rb_dev_release")

    def dev_cache_trim(self, keep_bytes=0):
        self._chk(self.L.rb_dev_cache_trim(self.ctx, C.c_uint64(keep_bytes)), "rb_dev_cache_trim")

    def dev_alloc_stats(self):
        """-> dict(live, cached, retired_va, va_cap, fallbacks): rb_dev_alloc_stats"""
        o = (C.c_uint64 * 5)()
        self._chk(self.L.rb_dev_alloc_stats(self.ctx, o), "rb_dev_alloc_stats")
        return dict(live=int(o[0]), cached=int(o[1]), retired_va=int(o[2]), va_cap=int(o[3]), fallbacks=int(o[4]))

    def text_scratch_bytes(self, n):
        f = self.L.rb_text_scratch_bytes
        f.restype = C.c_size_t
        return int(f(C.c_uint64(n)))

    def plan_create(self, op_off, contig, w_contig=None, w_st=None, w_en=None):
        op_off, contig = _arr(op_off, np.uint64), _arr(contig, np.uint32)
        nw = 0 if w_st is None else len(w_st)
        wc = _arr(w_contig if nw else np.zeros(0), np.uint32)
        ws = _arr(w_st if nw else np.zeros(0), np.uint64)
        we = _arr(w_en if nw else np.zeros(0), np.uint64)
        plan = C.c_void_p()
        self._chk(self.L.rb_plan_create(self.ctx, C.c_uint64(len(contig)), _p(op_off), _p(contig), C.c_uint64(nw),
                                        _p(wc), _p(ws), _p(we), C.byref(plan)), "rb_plan_create")
        return plan

    def plan_destroy(self, plan):
        self.L.rb_plan_destroy(plan)

    def plan_out_capacity(self, plan, for_break=False):
        return int(self.L.rb_plan_out_capacity(plan, C.c_int(1 if for_break else 0)))

    def plan_workspace_bytes(self, plan, rows_cap):
        return int(self.L.rb_plan_workspace_bytes(plan, C.c_uint64(rows_cap)))

    def dev_box_probe(self, src_ptr, src_bytes, dst0_ptr, dst1_ptr, reps=10, scatter=False):
        """-> (ms per launch, shader MHz held): the clip kernel's memory mix without its instructions (diagnostics)."""
        ms, mhz = C.c_double(0), C.c_double(0)
        self._chk(self.L.rb_dev_box_probe(self.ctx, C.c_void_p(src_ptr), C.c_uint64(src_bytes), C.c_void_p(dst0_ptr), C.c_void_p(dst1_ptr),
                                          C.c_int(reps), C.c_int(int(scatter)), C.byref(ms), C.byref(mhz)), "rb_dev_box_probe")
        return ms.value, mhz.value

    def plan_diag_stamps_offset(self, plan, rows_cap):
        return int(self.L.rb_plan_diag_stamps_offset(plan, C.c_uint64(rows_cap)))

    def dev_liftover(self, plan, view, norm_ptr, policy, ws_ptr, rows_ptr, rows_cap, out_ptr, out_cap, counters_ptr):
        self._chk(self.L.rb_dev_liftover(self.ctx, plan, C.byref(view), C.c_void_p(norm_ptr), C.c_int(policy),
                                         C.c_void_p(ws_ptr), C.c_void_p(rows_ptr), C.c_uint64(rows_cap),
                                         C.c_void_p(out_ptr), C.c_uint64(out_cap), C.c_void_p(counters_ptr)),
                  "rb_dev_liftover")

    def dev_break(self, plan, view, norm_ptr, max_size, policy, ws_ptr, rows_ptr, rows_cap, out_ptr, out_cap,
                  counters_ptr):
        self._chk(self.L.rb_dev_break(self.ctx, plan, C.byref(view), C.c_void_p(norm_ptr), C.c_uint32(max_size),
                                      C.c_int(policy), C.c_void_p(ws_ptr), C.c_void_p(rows_ptr), C.c_uint64(rows_cap),
                                      C.c_void_p(out_ptr), C.c_uint64(out_cap), C.c_void_p(counters_ptr)),
                  "rb_dev_break")

    def dev_stats_rows(self, view, rows_ptr, n_rows, out_ptr, stats_ptr):
        """rb_dev_stats_rows on device addresses: one reduce row (REDUCE_DT) per hit row, from the clip where it lies (plain ops in out_ops, or a
        descriptor into the batch of `view`); enqueues on the context's stream"""
        self._chk(self.L.rb_dev_stats_rows(self.ctx, C.byref(view), C.c_void_p(rows_ptr or 0), C.c_uint64(n_rows), C.c_void_p(out_ptr or 0),
                                           C.c_void_p(stats_ptr or 0)), "rb_dev_stats_rows")

    def stats_rows(self, ops, op_off, rows, out_ops):
        """rb_dev_stats_rows on host arrays (ops / op_off: the batch descriptor rows point into, op_off a table of starts; rows: HIT_DT;
        out_ops: what the rows' out_off index): uploads, runs, downloads -> REDUCE_DT [len(rows)]"""
        rows = _arr(rows, HIT_DT)

        def padded(a):  # readable up to the next multiple of four words
            a = _arr(a, np.uint32)
            return np.concatenate([a, np.zeros(-len(a) % 4 + 4, np.uint32)])
        ops, out_ops, op_off = padded(ops), padded(out_ops), _arr(op_off, np.uint64)
        stats = np.zeros(len(rows), REDUCE_DT)
        bufs = []
        try:
            for a in (ops, op_off, rows, out_ops, stats):
                bufs.append(self.dev_alloc(max(a.nbytes, 256)))
                if a.nbytes and a is not stats:
                    self._chk(self.L.rb_dev_upload(self.ctx, C.c_void_p(bufs[-1]), _p(a), C.c_size_t(a.nbytes)), "rb_dev_upload")
            view = self.batch_view(max(len(op_off) - 1, 0), len(ops), bufs[0], bufs[1], 0, 0, 0, 0, 0, 0)
            self.dev_stats_rows(view, bufs[2], len(rows), bufs[3], bufs[4])
            if stats.nbytes:
                self._chk(self.L.rb_dev_download(self.ctx, _p(stats), C.c_void_p(bufs[4]), C.c_size_t(stats.nbytes)), "rb_dev_download")
            return stats
        finally:
            self.sync()
            for b in bufs:
                self.dev_free(b)

    # ---- MD strings and query spans of alignment records (k_alnstats.hip) ----
    def _up(self, bufs, a, n_bytes=None):
        """a device buffer of n_bytes (at least the array's; tracked in bufs) holding the host array; -> address"""
        bufs.append(self.dev_alloc(max(a.nbytes if n_bytes is None else n_bytes, 256)))
        if a.nbytes:
            self._chk(self.L.rb_dev_upload(self.ctx, C.c_void_p(bufs[-1]), _p(a), C.c_size_t(a.nbytes)), "rb_dev_upload")
        return bufs[-1]

    def _down(self, a, ptr):
        if a.nbytes:
            self._chk(self.L.rb_dev_download(self.ctx, _p(a), C.c_void_p(ptr), C.c_size_t(a.nbytes)), "rb_dev_download")
        return a

    def dev_parse_md(self, text_ptr, md_off_ptr, md_end_ptr, n, out_ptr, status_ptr):
        """rb_dev_parse_md on device addresses; enqueues on the context's stream"""
        v = C.c_void_p
        self._chk(self.L.rb_dev_parse_md(self.ctx, v(text_ptr or 0), v(md_off_ptr or 0), v(md_end_ptr or 0), C.c_uint64(n), v(out_ptr or 0),
                                         v(status_ptr or 0)), "rb_dev_parse_md")

    def dev_aln_stats(self, view, reduce_ptr, pos_ptr, flag_ptr, l_seq_ptr, md_ptr, md_status_ptr, has_md_ptr, rows_ptr):
        """rb_dev_aln_stats on device addresses (view: ops and op_off of the batch); enqueues on the context's stream"""
        v = C.c_void_p
        self._chk(self.L.rb_dev_aln_stats(self.ctx, C.byref(view), v(reduce_ptr or 0), v(pos_ptr or 0), v(flag_ptr or 0), v(l_seq_ptr or 0),
                                          v(md_ptr or 0), v(md_status_ptr or 0), v(has_md_ptr or 0), v(rows_ptr or 0)), "rb_dev_aln_stats")

    def parse_md(self, text, md_off, md_end, guard=0):
        """rb_dev_parse_md on host arrays: text (bytes-like; padded here to the slack the call asks for), the strings' extents
        -> (out u32 [n + guard, 4], status u8 [n + guard]); the `guard` entries behind the n results were filled with 0xA5 before the call
        (the tests look at them afterwards)"""
        text = np.frombuffer(bytes(text), np.uint8)
        text = np.concatenate([text, np.full(-len(text) % 16, 0x5E, np.uint8)])  # (slack bytes: carets, which the call must not see)
        md_off, md_end = _arr(md_off, np.uint64), _arr(md_end, np.uint64)
        n = len(md_off)
        out, status = np.full((n + guard, 4), 0xA5A5A5A5, np.uint32), np.full(n + guard, 0xA5, np.uint8)
        bufs = []
        try:
            d = [self._up(bufs, a) for a in (text, md_off, md_end, out, status)]
            self.dev_parse_md(d[0], d[1], d[2], n, d[3], d[4])
            return self._down(out, d[3]), self._down(status, d[4])
        finally:
            self.sync()
            for b in bufs:
                self.dev_free(b)

    def host_parse_md(self, text, md_off, md_end):
        """rb_host_parse_md -> (out u32 [n, 4], status u8 [n])"""
        text = np.frombuffer(bytes(text), np.uint8)
        md_off, md_end = _arr(md_off, np.uint64), _arr(md_end, np.uint64)
        n = len(md_off)
        out, status = np.zeros((n, 4), np.uint32), np.zeros(n, np.uint8)
        self._chk(self.L.rb_host_parse_md(self.ctx, _p(text), C.c_uint64(len(text)), _p(md_off), _p(md_end), C.c_uint64(n), _p(out), _p(status)),
                  "rb_host_parse_md")
        return out, status

    def _aln_cols(self, n, pos, flag, l_seq, md, md_status, has_md):
        cols = [_arr(pos, np.int64), _arr(flag, np.uint32), _arr(l_seq, np.uint32)]
        cols += [None if has_md is None else _arr(md, np.uint32).reshape(-1), None if has_md is None or md_status is None else _arr(md_status, np.uint8),
                 None if has_md is None else _arr(has_md, np.uint8)]
        assert all(c is None or len(c) == (4 * n if i == 3 else n) for i, c in enumerate(cols)), "one entry per alignment (four per MD)"
        return cols

    def aln_stats(self, ops, op_off, reduce_rows, pos, flag, l_seq, md=None, md_status=None, has_md=None, guard=0):
        """rb_dev_aln_stats on host arrays (reduce_rows: REDUCE_DT, the record scan's rows of the batch with all coordinates zero; md [n, 4] /
        md_status / has_md: rb_dev_parse_md's outputs, or has_md None: no record has an MD) -> ALN_DT [n + guard]; the guard rows were
        filled with 0xA5 before the call"""
        ops, op_off, red = _arr(ops, np.uint32), _arr(op_off, np.uint64), _arr(reduce_rows, REDUCE_DT)
        n = len(op_off) - 1
        cols = self._aln_cols(n, pos, flag, l_seq, md, md_status, has_md)
        rows = np.frombuffer(np.full((n + guard) * ALN_DT.itemsize, 0xA5, np.uint8).tobytes(), ALN_DT).copy()
        bufs = []
        try:
            d = [0 if a is None else self._up(bufs, a) for a in [ops, op_off, red] + cols + [rows]]
            view = self.batch_view(n, len(ops), d[0], d[1], 0, 0, 0, 0, 0, 0)
            self.dev_aln_stats(view, *d[2:10])
            return self._down(rows, d[9])
        finally:
            self.sync()
            for b in bufs:
                self.dev_free(b)

    def host_aln_stats(self, ops, op_off, reduce_rows, pos, flag, l_seq, md=None, md_status=None, has_md=None):
        """rb_host_aln_stats -> ALN_DT [n]"""
        ops, op_off, red = _arr(ops, np.uint32), _arr(op_off, np.uint64), _arr(reduce_rows, REDUCE_DT)
        n = len(op_off) - 1
        cols = self._aln_cols(n, pos, flag, l_seq, md, md_status, has_md)
        rows = np.zeros(n, ALN_DT)
        self._chk(self.L.rb_host_aln_stats(self.ctx, C.c_uint64(n), _p(ops), _p(op_off), _p(red), *map(_p, cols), _p(rows)), "rb_host_aln_stats")
        return rows

    def bam_scratch_bytes(self, n):
        f = self.L.rb_bam_scratch_bytes
        f.restype = C.c_size_t
        return int(f(C.c_uint64(n)))

    def dev_bam_records(self, data_ptr, rec_off_ptr, rec_len_ptr, n, tid_ptr, pos_ptr, flag_ptr, l_seq_ptr, has_md_ptr, md_off_ptr, md_end_ptr, op_off_ptr,
                        ops_ptr, ops_cap, status_ptr, scratch_ptr):
        """rb_dev_bam_records on device addresses; enqueues on the context's stream"""
        v = C.c_void_p
        self._chk(self.L.rb_dev_bam_records(self.ctx, v(data_ptr or 0), v(rec_off_ptr or 0), v(rec_len_ptr or 0), C.c_uint64(n), v(tid_ptr or 0),
                                            v(pos_ptr or 0), v(flag_ptr or 0), v(l_seq_ptr or 0), v(has_md_ptr or 0), v(md_off_ptr or 0), v(md_end_ptr or 0),
                                            v(op_off_ptr or 0), v(ops_ptr or 0), C.c_uint64(ops_cap), v(status_ptr or 0), v(scratch_ptr or 0)),
                  "rb_dev_bam_records")

    @staticmethod
    def _bam_cols(n, guard, fill):
        mk = (lambda k, dt: np.frombuffer(np.full((k + guard) * np.dtype(dt).itemsize, 0xA5, np.uint8).tobytes(), dt).copy()) if fill else \
            (lambda k, dt: np.zeros(k, dt))
        return dict(tid=mk(n, np.int32), pos=mk(n, np.int64), flag=mk(n, np.uint32), l_seq=mk(n, np.uint32), has_md=mk(n, np.uint8), md_off=mk(n, np.uint64),
                    md_end=mk(n, np.uint64), op_off=mk(n + 1, np.uint64), status=mk(n, np.uint8))

    def bam_records(self, data, rec_off, rec_len, ops_cap=None, guard=0, keep=False, ops_fill=0xA5A5A5A5):
        """rb_dev_bam_records on host arrays: data (bytes-like; padded here to the slack the call asks for with 0xA5, which is no NUL), the
        records' places -> dict(tid, pos, flag, l_seq, has_md, md_off, md_end, status [n + guard], op_off [n + 1 + guard], ops u32
        [ops_cap + guard]); ops_cap None: (bytes of data) / 4.  The `guard` entries behind every array were filled with 0xA5 before the
        call, and all of ops with ops_fill.  keep: the device buffers stay (dict key "dev": name -> address, "free": call it when done) for
        calls that go on with the columns where they lie."""
        data = np.frombuffer(bytes(data), np.uint8)
        n_bytes = len(data)
        data = np.concatenate([data, np.full(-len(data) % 16, 0xA5, np.uint8)])
        rec_off, rec_len = _arr(rec_off, np.uint64), _arr(rec_len, np.uint32)
        n = len(rec_off)
        cap = n_bytes // 4 if ops_cap is None else int(ops_cap)
        out = self._bam_cols(n, guard, True)
        out["ops"] = np.full(cap + guard, ops_fill, np.uint32)
        names = ("tid", "pos", "flag", "l_seq", "has_md", "md_off", "md_end", "op_off", "ops", "status")
        bufs = []
        try:
            d = {k: self._up(bufs, a) for k, a in (("data", data), ("rec_off", rec_off), ("rec_len", rec_len))}
            d.update({k: self._up(bufs, out[k]) for k in names})
            d["scratch"] = self._up(bufs, np.zeros(self.bam_scratch_bytes(n), np.uint8))
            self.dev_bam_records(d["data"], d["rec_off"], d["rec_len"], n, *[d[k] for k in names[:9]], cap, d["status"], d["scratch"])
            for k in names:
                self._down(out[k], d[k])
            self.sync()
            if keep:
                out["dev"], bufs_kept = d, list(bufs)
                out["free"] = lambda: [self.dev_free(b) for b in bufs_kept]
                bufs = []
            return out
        finally:
            self.sync()
            for b in bufs:
                self.dev_free(b)

    def host_bam_records(self, data, rec_off, rec_len, ops_cap=None):
        """rb_host_bam_records -> the same dict without guards (ops [ops_cap], zero behind what the call wrote)"""
        data = np.frombuffer(bytes(data), np.uint8)
        rec_off, rec_len = _arr(rec_off, np.uint64), _arr(rec_len, np.uint32)
        n = len(rec_off)
        cap = len(data) // 4 if ops_cap is None else int(ops_cap)
        out = self._bam_cols(n, 0, False)
        out["ops"] = np.zeros(cap, np.uint32)
        self._chk(self.L.rb_host_bam_records(self.ctx, _p(data), C.c_uint64(len(data)), _p(rec_off), _p(rec_len), C.c_uint64(n),
                                             *[_p(out[k]) for k in ("tid", "pos", "flag", "l_seq", "has_md", "md_off", "md_end", "op_off", "ops")],
                                             C.c_uint64(cap), _p(out["status"])), "rb_host_bam_records")
        return out

    # ---- the per-read index of nucfreq (k_bamreads.hip) ----
    def bam_reads_scratch_bytes(self, n):
        f = self.L.rb_bam_reads_scratch_bytes
        f.restype = C.c_size_t
        return int(f(C.c_uint64(n)))

    def dev_bam_reads(self, data_ptr, rec_off_ptr, rec_len_ptr, n, tid_ptr, pos_ptr, flag_ptr, op_off_ptr, ops_ptr, status_ptr, seq_off_ptr,
                      start_key_ptr, end_key_pmax_ptr, first_unsorted_ptr, scratch_ptr, check=True):
        """rb_dev_bam_reads on device addresses; enqueues on the context's stream.  Returns the call's return value (check=False: without
        raising)."""
        v = C.c_void_p
        rc = self.L.rb_dev_bam_reads(self.ctx, v(data_ptr or 0), v(rec_off_ptr or 0), v(rec_len_ptr or 0), C.c_uint64(n), v(tid_ptr or 0), v(pos_ptr or 0),
                                     v(flag_ptr or 0), v(op_off_ptr or 0), v(ops_ptr or 0), v(status_ptr or 0), v(seq_off_ptr or 0), v(start_key_ptr or 0),
                                     v(end_key_pmax_ptr or 0), v(first_unsorted_ptr or 0), v(scratch_ptr or 0))
        if check:
            self._chk(rc, "rb_dev_bam_reads")
        return int(rc)

    def bam_reads(self, data, rec_off, rec_len, guard=0, keep=False):
        """rb_dev_bam_records, then rb_dev_bam_reads on its columns where they lie -> the dict of bam_records() plus seq_off, start_key,
        end_key_pmax [n + guard] and first_unsorted [1 + guard] (every entry 0xA5 before the call, scratch too; ops was filled with 0xA0A0A0A0, an M of
        length 0xA0A0A0A: a word behind a record's last op that got into its sum would show).  keep: as bam_records()."""
        out = self.bam_records(data, rec_off, rec_len, guard=guard, keep=True, ops_fill=0xA0A0A0A0)
        n = len(out["status"]) - guard
        d, bufs = out["dev"], []
        names = ("seq_off", "start_key", "end_key_pmax", "first_unsorted")
        try:
            for k in names:
                out[k] = np.full((1 if k == "first_unsorted" else n) + guard, 0xA5A5A5A5A5A5A5A5, np.uint64)
                d[k] = self._up(bufs, out[k])
            d["reads_scratch"] = self._up(bufs, np.full(self.bam_reads_scratch_bytes(n) + 256, 0xA5, np.uint8))
            scr = (d["reads_scratch"] + 255) & ~255
            self.dev_bam_reads(d["data"], d["rec_off"], d["rec_len"], n, d["tid"], d["pos"], d["flag"], d["op_off"], d["ops"], d["status"], d["seq_off"],
                               d["start_key"], d["end_key_pmax"], d["first_unsorted"], scr)
            for k in names:
                self._down(out[k], d[k])
            self.sync()
            if keep:
                free0, kept = out["free"], list(bufs)
                out["free"] = lambda: (free0(), [self.dev_free(b) for b in kept])
                bufs = []
            return out
        finally:
            self.sync()
            for b in bufs:
                self.dev_free(b)
            if not keep:
                out["free"]()

    def host_bam_reads(self, data, rec_off, rec_len, ops_cap=None):
        """rb_host_bam_reads -> the dict of host_bam_records() plus seq_off, start_key, end_key_pmax [n] and first_unsorted [1]"""
        data = np.frombuffer(bytes(data), np.uint8)
        rec_off, rec_len = _arr(rec_off, np.uint64), _arr(rec_len, np.uint32)
        n = len(rec_off)
        cap = len(data) // 4 if ops_cap is None else int(ops_cap)
        out = self._bam_cols(n, 0, False)
        out["ops"] = np.zeros(cap, np.uint32)
        for k in ("seq_off", "start_key", "end_key_pmax"):
            out[k] = np.zeros(n, np.uint64)
        out["first_unsorted"] = np.zeros(1, np.uint64)
        self._chk(self.L.rb_host_bam_reads(self.ctx, _p(data), C.c_uint64(len(data)), _p(rec_off), _p(rec_len), C.c_uint64(n),
                                           *[_p(out[k]) for k in ("tid", "pos", "flag", "l_seq", "has_md", "md_off", "md_end", "op_off", "ops")],
                                           C.c_uint64(cap), _p(out["status"]), _p(out["seq_off"]), _p(out["start_key"]), _p(out["end_key_pmax"]),
                                           _p(out["first_unsorted"])), "rb_host_bam_reads")
        return out

    def rows_to_batch_scratch_bytes(self, n_rows):
        f = self.L.rb_rows_to_batch_scratch_bytes
        f.restype = C.c_size_t
        return int(f(C.c_uint64(n_rows)))

    def dev_rows_to_batch(self, view, rows_ptr, n_rows, out_ptr, pieces_cap, ops_cap, new_ops_ptr, new_off_ptr, coord_ptrs, strand_ptr, contig_ptr,
                          parent_ptr, info_ptr, scratch_ptr):
        """rb_dev_rows_to_batch on device addresses (coord_ptrs = t_st, t_en, q_st, q_en of the pieces; new_ops_ptr 0: sizes only, the other
        outputs may then be 0 too); enqueues on the context's stream"""
        t_st, t_en, q_st, q_en = coord_ptrs if coord_ptrs else (0, 0, 0, 0)
        v = C.c_void_p
        self._chk(self.L.rb_dev_rows_to_batch(self.ctx, C.byref(view), v(rows_ptr or 0), C.c_uint64(n_rows), v(out_ptr or 0), C.c_uint64(pieces_cap),
                                              C.c_uint64(ops_cap), v(new_ops_ptr or 0), v(new_off_ptr or 0), v(t_st or 0), v(t_en or 0), v(q_st or 0),
                                              v(q_en or 0), v(strand_ptr or 0), v(contig_ptr or 0), v(parent_ptr or 0), v(info_ptr), v(scratch_ptr or 0)),
                  "rb_dev_rows_to_batch")

    def rows_to_batch(self, ops, op_off, strand, contig, rows, out_ops):
        """rb_dev_rows_to_batch on host arrays (ops / op_off / strand / contig: the batch the rows came from, op_off a table of starts; rows:
        HIT_DT; out_ops: what the rows' out_off index): a sizes-only call, then the fill with exactly those sizes -> (dict of the piece
        batch's arrays ops, op_off, t_st, t_en, q_st, q_en, strand, contig, parent; info PIECES_INFO_DT)"""
        rows = _arr(rows, HIT_DT)

        def padded(a):  # readable up to the next multiple of four words
            a = _arr(a, np.uint32)
            return np.concatenate([a, np.zeros(-len(a) % 4 + 4, np.uint32)])
        ops, out_ops, op_off = padded(ops), padded(out_ops), _arr(op_off, np.uint64)
        strand, contig = _arr(strand, np.uint8), _arr(contig, np.uint32)
        bufs = []

        def dev(n_bytes, src=None):
            bufs.append(self.dev_alloc(max(n_bytes, 256)))
            if src is not None and src.nbytes:
                self._chk(self.L.rb_dev_upload(self.ctx, C.c_void_p(bufs[-1]), _p(src), C.c_size_t(src.nbytes)), "rb_dev_upload")
            return bufs[-1]

        def down(ptr, n, dt):
            a = np.zeros(n, dt)
            if a.nbytes:
                self._chk(self.L.rb_dev_download(self.ctx, _p(a), C.c_void_p(ptr), C.c_size_t(a.nbytes)), "rb_dev_download")
            return a
        try:
            view = self.batch_view(max(len(op_off) - 1, 0), len(ops), dev(ops.nbytes, ops), dev(op_off.nbytes, op_off), 0, 0, 0, 0,
                                   dev(strand.nbytes, strand), dev(contig.nbytes, contig))
            d_rows, d_out, d_info = dev(rows.nbytes, rows), dev(out_ops.nbytes, out_ops), dev(64)
            d_scr = dev(self.rows_to_batch_scratch_bytes(len(rows)))
            self.dev_rows_to_batch(view, d_rows, len(rows), d_out, 0, 0, 0, 0, None, 0, 0, 0, d_info, d_scr)
            info = down(d_info, 1, PIECES_INFO_DT)[0]
            n_p, n_o = int(info["n_pieces"]), int(info["n_ops"])
            d_new, d_off = dev(4 * n_o + 128), dev(8 * (n_p + 1))
            d_c = [dev(8 * n_p) for _ in range(4)]
            d_s, d_ct, d_par = dev(n_p), dev(4 * n_p), dev(4 * n_p)
            self.dev_rows_to_batch(view, d_rows, len(rows), d_out, n_p, n_o, d_new, d_off, d_c, d_s, d_ct, d_par, d_info, d_scr)
            info = down(d_info, 1, PIECES_INFO_DT)[0]
            b = dict(ops=down(d_new, n_o, np.uint32), op_off=down(d_off, n_p + 1, np.uint64), strand=down(d_s, n_p, np.uint8),
                     contig=down(d_ct, n_p, np.uint32), parent=down(d_par, n_p, np.uint32))
            for k, ptr in zip(("t_st", "t_en", "q_st", "q_en"), d_c):
                b[k] = down(ptr, n_p, np.uint64)
            return b, info
        finally:
            self.sync()
            for x in bufs:
                self.dev_free(x)

    def pairs_scratch_bytes(self, n_keys, n_rows):
        f = self.L.rb_pairs_scratch_bytes
        f.restype = C.c_size_t
        return int(f(C.c_uint64(n_keys), C.c_uint64(n_rows)))

    def dev_pairs_rows(self, rows_ptr, n_rows, rec_key_ptr, rec_q_len_ptr, strand_ptr, n_rec, n_keys, mode, paired_len, min_aln, min_query, rows_out_ptr,
                       rows_cap, key_flip_ptr, info_ptr, scratch_ptr):
        """orient / filter over hit rows where they lie (every pointer a device address): the kept rows, dense, to rows_out_ptr[rows_cap], a
        byte per key to key_flip_ptr, PAIRS_INFO_DT to info_ptr; enqueues on the context's stream"""
        v = C.c_void_p
        self._chk(self.L.rb_dev_pairs_rows(self.ctx, v(rows_ptr or 0), C.c_uint64(n_rows), v(rec_key_ptr or 0), v(rec_q_len_ptr or 0), v(strand_ptr or 0),
                                           C.c_uint64(n_rec), C.c_uint64(n_keys), C.c_uint32(mode), C.c_uint64(paired_len), C.c_uint64(min_aln),
                                           C.c_uint64(min_query), v(rows_out_ptr or 0), C.c_uint64(rows_cap), v(key_flip_ptr or 0), v(info_ptr),
                                           v(scratch_ptr or 0)), "rb_dev_pairs_rows")

    def pairs_rows(self, rows, rec_key, rec_q_len, strand, n_keys, mode, paired_len=0, min_aln=0, min_query=0):
        """rb_dev_pairs_rows on host arrays (rows: HIT_DT): uploads, runs with room for every row, downloads
        -> (rows_out HIT_DT [n_kept], key_flip u8 [n_keys], info PAIRS_INFO_DT)"""
        rows, rec_key = _arr(rows, HIT_DT), _arr(rec_key, np.uint32)
        rec_q_len, strand = _arr(rec_q_len, np.uint64), _arr(strand, np.uint8)
        n_keys = int(n_keys)
        bufs = []

        def dev(n_bytes, src=None):
            bufs.append(self.dev_alloc(max(n_bytes, 256)))
            if src is not None and src.nbytes:
                self._chk(self.L.rb_dev_upload(self.ctx, C.c_void_p(bufs[-1]), _p(src), C.c_size_t(src.nbytes)), "rb_dev_upload")
            return bufs[-1]

        def down(ptr, n, dt):
            a = np.zeros(n, dt)
            if a.nbytes:
                self._chk(self.L.rb_dev_download(self.ctx, _p(a), C.c_void_p(ptr), C.c_size_t(a.nbytes)), "rb_dev_download")
            return a
        try:
            d_rows, d_key, d_ql, d_s = dev(rows.nbytes, rows), dev(rec_key.nbytes, rec_key), dev(rec_q_len.nbytes, rec_q_len), dev(strand.nbytes, strand)
            d_out, d_flip, d_info = dev(rows.nbytes), dev(n_keys), dev(64)
            d_scr = dev(self.pairs_scratch_bytes(n_keys, len(rows)))
            self.dev_pairs_rows(d_rows, len(rows), d_key, d_ql, d_s, len(rec_key), n_keys, mode, paired_len, min_aln, min_query, d_out, len(rows), d_flip,
                                d_info, d_scr)
            info = down(d_info, 1, PAIRS_INFO_DT)[0]
            return down(d_out, int(info["n_kept"]), HIT_DT), down(d_flip, n_keys, np.uint8), info
        finally:
            self.sync()
            for b in bufs:
                self.dev_free(b)

    def pairs_records_scratch_bytes(self, n_keys, n_rec):
        f = self.L.rb_pairs_records_scratch_bytes
        f.restype = C.c_size_t
        return int(f(C.c_uint64(n_keys), C.c_uint64(n_rec)))

    def dev_pairs_records(self, t_st, t_en, q_st, q_en, strand, rec_key, rec_q_len, n_rec, n_keys, mode, paired_len, min_aln, min_query, kept, kept_cap,
                          q_st_out, q_en_out, key_flip, key_order, info, scratch):
        """orient / filter over the records of a resident batch (every pointer a device address; kept, q_st_out / q_en_out, key_order may be 0);
        enqueues on the context's stream -> the return code (RB_E_INVALID = -1 for what the call refuses): the caller checks it"""
        v = C.c_void_p
        return int(self.L.rb_dev_pairs_records(self.ctx, v(t_st or 0), v(t_en or 0), v(q_st or 0), v(q_en or 0), v(strand or 0), v(rec_key or 0),
                                               v(rec_q_len or 0), C.c_uint64(n_rec), C.c_uint64(n_keys), C.c_uint32(mode), C.c_uint64(paired_len),
                                               C.c_uint64(min_aln), C.c_uint64(min_query), v(kept or 0), C.c_uint64(kept_cap), v(q_st_out or 0),
                                               v(q_en_out or 0), v(key_flip or 0), v(key_order or 0), v(info or 0), v(scratch or 0)))

    def pairs_records(self, t_st, t_en, q_st, q_en, strand, rec_key, rec_q_len, n_keys, mode, paired_len=0, min_aln=0, min_query=0):
        """rb_dev_pairs_records on host arrays: uploads, runs with room for every record, downloads
        -> dict(kept u32 [n_kept], q_st, q_en u64 [n_rec], key_flip u8 [n_keys], key_order u64 [n_keys], info PAIRS_INFO_DT)"""
        cols = _pairs_records_cols(t_st, t_en, q_st, q_en, strand, rec_key, rec_q_len)
        n, n_keys = len(cols[0]), int(n_keys)
        bufs = []

        def dev(n_bytes, src=None):
            bufs.append(self.dev_alloc(max(n_bytes, 256)))
            if src is not None and src.nbytes:
                self._chk(self.L.rb_dev_upload(self.ctx, C.c_void_p(bufs[-1]), _p(src), C.c_size_t(src.nbytes)), "rb_dev_upload")
            return bufs[-1]

        def down(ptr, k, dt):
            a = np.zeros(k, dt)
            if a.nbytes:
                self._chk(self.L.rb_dev_download(self.ctx, _p(a), C.c_void_p(ptr), C.c_size_t(a.nbytes)), "rb_dev_download")
            return a
        try:
            d_cols = [dev(c.nbytes, c) for c in cols]
            d_kept, d_qs, d_qe, d_flip, d_ord, d_info = dev(4 * n), dev(8 * n), dev(8 * n), dev(n_keys), dev(8 * n_keys), dev(64)
            d_scr = dev(self.pairs_records_scratch_bytes(n_keys, n))
            self._chk(self.dev_pairs_records(*d_cols, n, n_keys, mode, paired_len, min_aln, min_query, d_kept, n, d_qs, d_qe, d_flip, d_ord, d_info, d_scr),
                      "rb_dev_pairs_records")
            info = down(d_info, 1, PAIRS_INFO_DT)[0]
            return dict(kept=down(d_kept, int(info["n_kept"]), np.uint32), q_st=down(d_qs, n, np.uint64), q_en=down(d_qe, n, np.uint64),
                        key_flip=down(d_flip, n_keys, np.uint8), key_order=down(d_ord, n_keys, np.uint64), info=info)
        finally:
            self.sync()
            for b in bufs:
                self.dev_free(b)

    def pairs_text(self, text, cig_off, cig_end, t_st, t_en, q_st, q_en, strand, rec_key, rec_q_len, n_keys, mode, paired_len=0, min_aln=0, min_query=0):
        """rb_host_pairs_text: `rb orient` / `rb filter` on the records of a file whose text is `text` (bytes; record r's cg:Z: value is
        text[cig_off[r]:cig_end[r]]) -> dict(cig_status u8 [n_rec], reduce REDUCE_DT [n_rec], kept u32 [n_kept], q_st, q_en u64 [n_rec],
        key_flip u8, key_order u64 [n_keys], cigars: list of bytes per kept record, declined int)"""
        cols = _pairs_records_cols(t_st, t_en, q_st, q_en, strand, rec_key, rec_q_len)
        coff, cend = _arr(cig_off, np.uint64), _arr(cig_end, np.uint64)
        n, n_keys = len(cols[0]), int(n_keys)
        buf = np.frombuffer(bytes(text) + b"\0" * 32, dtype=np.uint8).copy()
        status, red = np.zeros(max(n, 1), np.uint8), np.zeros(n, REDUCE_DT)
        qs, qe, flip, order = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n_keys, np.uint8), np.zeros(n_keys, np.uint64)
        kept, toff, out = C.c_void_p(), C.c_void_p(), C.c_void_p()
        nk, declined = C.c_uint64(), C.c_int()
        t_st_, t_en_, q_st_, q_en_, strand_, key_, qlen_ = cols
        self._chk(self.L.rb_host_pairs_text(self.ctx, C.c_uint64(n), _p(buf), C.c_uint64(len(text)), _p(coff), _p(cend), _p(t_st_), _p(t_en_), _p(q_st_),
                                            _p(q_en_), _p(strand_), _p(key_), _p(qlen_), C.c_uint64(n_keys), C.c_uint32(mode), C.c_uint64(paired_len),
                                            C.c_uint64(min_aln), C.c_uint64(min_query), _p(status), _p(red), C.byref(kept), C.byref(nk), _p(qs), _p(qe),
                                            _p(flip), _p(order), C.byref(toff), C.byref(out), C.byref(declined)), "rb_host_pairs_text")

        def take(ptr, k, dt):
            r = np.frombuffer((C.c_char * (k * np.dtype(dt).itemsize)).from_address(ptr.value), dtype=dt).copy() if k and ptr.value else np.zeros(0, dt)
            self.L.rb_host_free(ptr)
            return r
        k = int(nk.value)
        offs = take(toff, k + 1, np.uint64)
        body = take(out, int(offs[k]) if len(offs) > k else 0, np.uint8).tobytes()
        return dict(cig_status=status[:n], reduce=red, kept=take(kept, k, np.uint32), q_st=qs, q_en=qe, key_flip=flip, key_order=order,
                    cigars=[body[int(offs[i]):int(offs[i + 1])] for i in range(k)], declined=int(declined.value))

    def largest_scratch_bytes(self, n_keys):
        f = self.L.rb_largest_scratch_bytes
        f.restype = C.c_size_t
        return int(f(C.c_uint64(n_keys)))

    def dev_largest(self, rows_ptr, n_rows, win_key_ptr, rec_key_ptr, n_keys, sel_ptr, out_ptr, scratch_ptr):
        """liftover --largest over hit rows where they lie (every pointer a device address, rec_key_ptr may be 0); enqueues on the context's
        stream: sel_ptr[0 .. out_ptr[0]) = the winners' row indices in key order, out_ptr[1] = rows left out for their key"""
        self._chk(self.L.rb_dev_largest(self.ctx, C.c_void_p(rows_ptr or 0), C.c_uint64(n_rows), C.c_void_p(win_key_ptr or 0),
                                        C.c_void_p(rec_key_ptr or 0), C.c_uint64(n_keys), C.c_void_p(sel_ptr or 0), C.c_void_p(out_ptr),
                                        C.c_void_p(scratch_ptr or 0)), "rb_dev_largest")

    def largest(self, rows, win_key, rec_key, n_keys):
        """rb_dev_largest on host arrays (rows: HIT_DT; rec_key may be None): uploads, runs, downloads -> (sel u64 [n_sel], n_bad)"""
        rows, win_key = _arr(rows, HIT_DT), _arr(win_key, np.uint32)
        rec_key = None if rec_key is None else _arr(rec_key, np.uint32)
        n_keys = int(n_keys)
        bufs = []

        def dev(n_bytes, src=None):
            bufs.append(self.dev_alloc(max(n_bytes, 256)))
            if src is not None and src.nbytes:
                self._chk(self.L.rb_dev_upload(self.ctx, C.c_void_p(bufs[-1]), _p(src), C.c_size_t(src.nbytes)), "rb_dev_upload")
            return bufs[-1]
        try:
            d_rows, d_wk = dev(rows.nbytes, rows), dev(win_key.nbytes, win_key)
            d_rk = 0 if rec_key is None else dev(rec_key.nbytes, rec_key)
            d_sel, d_out, d_scr = dev(8 * n_keys), dev(16), dev(self.largest_scratch_bytes(n_keys))
            self.dev_largest(d_rows, len(rows), d_wk, d_rk, n_keys, d_sel, d_out, d_scr)
            out = np.zeros(2, np.uint64)
            self._chk(self.L.rb_dev_download(self.ctx, _p(out), C.c_void_p(d_out), C.c_size_t(16)), "rb_dev_download")
            sel = np.zeros(int(out[0]), np.uint64)
            if len(sel):
                self._chk(self.L.rb_dev_download(self.ctx, _p(sel), C.c_void_p(d_sel), C.c_size_t(sel.nbytes)), "rb_dev_download")
            return sel, int(out[1])
        finally:
            self.sync()
            for b in bufs:
                self.dev_free(b)

    # ---- host-buffer wrappers ----
    def scan_records(self, ops, op_off, t_st, t_en, q_st, q_en, strand):
        ops, op_off = _arr(ops, np.uint32), _arr(op_off, np.uint64)
        n = len(op_off) - 1
        ops = np.concatenate([ops, np.zeros(4, np.uint32)])
        red, norm = np.zeros(n, REDUCE_DT), np.zeros(n, NORM_DT)
        a = [_arr(x, np.uint64) for x in (t_st, t_en, q_st, q_en)]
        s = _arr(strand, np.uint8)
        self._chk(self.L.rb_host_scan_records(self.ctx, C.c_uint64(n), _p(ops), _p(op_off), *map(_p, a), _p(s),
                                              _p(red), _p(norm)), "rb_host_scan_records")
        return red, norm

    def _lift(self, fn, what, n, args):
        rows, out = C.c_void_p(), C.c_void_p()
        nr, no = C.c_uint64(), C.c_uint64()
        norm = np.zeros(n, NORM_DT)
        cnt = np.zeros(1, COUNTERS_DT)
        self._chk(fn(self.ctx, *args, _p(norm), C.byref(rows), C.byref(nr), C.byref(out), C.byref(no), _p(cnt)), what)

        def take(ptr, k, dt):
            if k == 0:
                r = np.zeros(0, dt)
            else:
                buf = (C.c_char * (k * np.dtype(dt).itemsize)).from_address(ptr.value)
                r = np.frombuffer(buf, dtype=dt).copy()
            self.L.rb_host_free(ptr)
            return r
        return take(rows, nr.value, HIT_DT), take(out, no.value, np.uint32), norm, cnt[0]

    def liftover(self, ops, op_off, t_st, t_en, q_st, q_en, strand, contig, w_contig, w_st, w_en,
                 policy=BSEARCH_MODERN):
        ops, op_off = _arr(ops, np.uint32), _arr(op_off, np.uint64)
        n = len(op_off) - 1
        ops = np.concatenate([ops, np.zeros(4, np.uint32)])
        a = [_arr(x, np.uint64) for x in (t_st, t_en, q_st, q_en)]
        s, c = _arr(strand, np.uint8), _arr(contig, np.uint32)
        wc, ws, we = _arr(w_contig, np.uint32), _arr(w_st, np.uint64), _arr(w_en, np.uint64)
        args = [C.c_uint64(n), _p(ops), _p(op_off), *map(_p, a), _p(s), _p(c), C.c_uint64(len(ws)), _p(wc), _p(ws),
                _p(we), C.c_int(policy)]
        return self._lift(self.L.rb_host_liftover, "rb_host_liftover", n, args)

    def break_paf(self, ops, op_off, t_st, t_en, q_st, q_en, strand, max_size, policy=BSEARCH_MODERN):
        ops, op_off = _arr(ops, np.uint32), _arr(op_off, np.uint64)
        n = len(op_off) - 1
        ops = np.concatenate([ops, np.zeros(4, np.uint32)])
        a = [_arr(x, np.uint64) for x in (t_st, t_en, q_st, q_en)]
        s = _arr(strand, np.uint8)
        args = [C.c_uint64(n), _p(ops), _p(op_off), *map(_p, a), _p(s), C.c_uint32(max_size), C.c_int(policy)]
        return self._lift(self.L.rb_host_break, "rb_host_break", n, args)

    def overlap_split(self, ops, op_off, t_st, t_en, q_st, q_en, strand, left, right, scores=(1, 1, 1),
                      policy=BSEARCH_MODERN):
        ops, op_off = _arr(ops, np.uint32), _arr(op_off, np.uint64)
        n = len(op_off) - 1
        ops = np.concatenate([ops, np.zeros(4, np.uint32)])
        a = [_arr(x, np.uint64) for x in (t_st, t_en, q_st, q_en)]
        s = _arr(strand, np.uint8)
        left, right = _arr(left, np.uint32), _arr(right, np.uint32)
        rows = np.zeros(len(left), PAIR_DT)
        out, no = C.c_void_p(), C.c_uint64()
        self._chk(self.L.rb_host_overlap_split(self.ctx, C.c_uint64(n), _p(ops), _p(op_off), *map(_p, a), _p(s),
                                               C.c_uint64(len(left)), _p(left), _p(right), C.c_int(scores[0]),
                                               C.c_int(scores[1]), C.c_int(scores[2]), C.c_int(policy), _p(rows),
                                               C.byref(out), C.byref(no)), "rb_host_overlap_split")
        if no.value:
            buf = (C.c_char * (no.value * 4)).from_address(out.value)
            o = np.frombuffer(buf, dtype=np.uint32).copy()
        else:
            o = np.zeros(0, np.uint32)
        self.L.rb_host_free(out)
        return rows, o

    def dev_swap(self, view, out_ptr):
        """rb_dev_swap on device addresses; out_ptr == view.ops swaps every record where it lies.  Enqueues on the context's stream.
        -> the return code (RB_E_INVALID = -1 for an out_ptr that overlaps the ops without being equal to them): the caller checks it"""
        return int(self.L.rb_dev_swap(self.ctx, C.byref(view), C.c_void_p(out_ptr)))

    def swap(self, ops, op_off, strand, in_place=False):
        ops, op_off, s = _arr(ops, np.uint32), _arr(op_off, np.uint64), _arr(strand, np.uint8)
        n = len(op_off) - 1
        if in_place:  # upload, rb_dev_swap with out_ops == ops, download
            buf = np.concatenate([ops, np.zeros(4, np.uint32)])
            bufs = [self.dev_alloc(max(a.nbytes, 256)) for a in (buf, op_off, s)]
            try:
                for d, a in zip(bufs, (buf, op_off, s)):
                    if a.nbytes:
                        self._chk(self.L.rb_dev_upload(self.ctx, C.c_void_p(d), _p(a), C.c_size_t(a.nbytes)), "rb_dev_upload")
                view = self.batch_view(n, int(op_off[n]) if n else 0, bufs[0], bufs[1], 0, 0, 0, 0, bufs[2], 0)
                self._chk(self.dev_swap(view, bufs[0]), "rb_dev_swap")
                self._chk(self.L.rb_dev_download(self.ctx, _p(buf), C.c_void_p(bufs[0]), C.c_size_t(buf.nbytes)), "rb_dev_download")
            finally:
                self.sync()
                for d in bufs:
                    self.dev_free(d)
            return buf[:len(ops)]
        out = np.zeros(len(ops) + 4, np.uint32)
        src = np.concatenate([ops, np.zeros(4, np.uint32)])
        self._chk(self.L.rb_host_swap(self.ctx, C.c_uint64(n), _p(src), _p(op_off), _p(s), _p(out)), "rb_host_swap")
        return out[:len(ops)]

    # ---- CIGAR text <-> packed ops (k_text.hip) ----
    def parse_cigars(self, cigars):
        """cigars: list of bytes / str (the cg:Z: values).  Returns (op_off, ops, status)."""
        bs = [c.encode() if isinstance(c, str) else bytes(c) for c in cigars]
        off = np.zeros(len(bs) + 1, np.uint64)
        if bs:
            off[1:] = np.cumsum([len(b) for b in bs], dtype=np.uint64)
        text = np.frombuffer(b"".join(bs) + b"\0" * 32, dtype=np.uint8).copy()
        return self.parse_cigar_text(text, off, None)

    def parse_cigar_text(self, text, text_off, text_end=None):
        text, text_off = _arr(text, np.uint8), _arr(text_off, np.uint64)
        n = len(text_off) - 1
        end = None if text_end is None else _arr(text_end, np.uint64)
        op_off = np.zeros(n + 1, np.uint64)
        status = np.zeros(max(n, 1), np.uint8)
        out = C.c_void_p()
        self._chk(self.L.rb_host_parse_cigars(self.ctx, _p(text), _p(text_off), _p(end) if end is not None else None,
                                              C.c_uint64(n), _p(op_off), C.byref(out), _p(status)), "rb_host_parse_cigars")
        n_ops = int(op_off[n])
        if n_ops:
            ops = np.frombuffer((C.c_char * (n_ops * 4)).from_address(out.value), dtype=np.uint32).copy()
        else:
            ops = np.zeros(0, np.uint32)
        self.L.rb_host_free(out)
        return op_off, ops, status[:n]

    def format_cigars(self, ops, first, count, first_len=None, last_len=None):
        """Items = runs ops[first[i] : first[i] + count[i]] with optional clipped first / last lengths.  Returns (text_off, text)."""
        ops, first, count = _arr(ops, np.uint32), _arr(first, np.uint64), _arr(count, np.uint32)
        n = len(first)
        fl = None if first_len is None else _arr(first_len, np.uint32)
        ll = None if last_len is None else _arr(last_len, np.uint32)
        toff = np.zeros(n + 1, np.uint64)
        out = C.c_void_p()
        src = np.concatenate([ops, np.zeros(4, np.uint32)])
        self._chk(self.L.rb_host_format_cigars(self.ctx, _p(src), C.c_uint64(len(ops)), C.c_uint64(n), _p(first), _p(count),
                                               _p(fl) if fl is not None else None, _p(ll) if ll is not None else None, _p(toff),
                                               C.byref(out)), "rb_host_format_cigars")
        nb = int(toff[n])
        text = bytes((C.c_char * nb).from_address(out.value)) if nb else b""
        self.L.rb_host_free(out)
        return toff, text


    # ---- nucfreq (k_nucfreq.hip) ----
    def nucfreq_workspace_bytes(self, n_reads, n_regions, n_pos):
        f = self.L.rb_nucfreq_workspace_bytes
        f.restype = C.c_size_t
        return int(f(C.c_uint64(n_reads), C.c_uint64(n_regions), C.c_uint64(n_pos)))

    def dev_nucfreq(self, n_reads, ops, op_off, seq, seq_off, l_seq, tid, pos, flag, n_regions, rg_tid, rg_st, rg_en, out_off, n_pos,
                    counts, status, counters, ws, ws_bytes):
        """every pointer argument is a device address (int); enqueues on the context's stream"""
        class View(C.Structure):
            _fields_ = [("n_reads", C.c_uint64), ("ops", C.c_void_p), ("op_off", C.c_void_p), ("seq", C.c_void_p), ("seq_off", C.c_void_p),
                        ("l_seq", C.c_void_p), ("tid", C.c_void_p), ("pos", C.c_void_p), ("flag", C.c_void_p)]
        v = View(n_reads, ops, op_off, seq, seq_off, l_seq, tid, pos, flag)
        self._chk(self.L.rb_dev_nucfreq(self.ctx, C.byref(v), C.c_uint64(n_regions), C.c_void_p(rg_tid), C.c_void_p(rg_st), C.c_void_p(rg_en),
                                        C.c_void_p(out_off), C.c_uint64(n_pos), C.c_void_p(counts), C.c_void_p(status), C.c_void_p(counters),
                                        C.c_void_p(ws), C.c_size_t(ws_bytes)), "rb_dev_nucfreq")

    def nucfreq(self, tid, pos, flag, op_off, ops, l_seq, seq_off, seq, rg_tid, rg_st, rg_en):
        """Reads (BAM file order) x regions -> (counts [n_positions, 4] u32 with NF_COVERED in bit 31 of column 0,
        read_status [n_reads], counters dict)."""
        tid, pos, flag = _arr(tid, np.int32), _arr(pos, np.int64), _arr(flag, np.uint32)
        op_off, ops = _arr(op_off, np.uint64), np.concatenate([_arr(ops, np.uint32), np.zeros(4, np.uint32)])
        l_seq, seq_off = _arr(l_seq, np.uint32), _arr(seq_off, np.uint64)
        seq = np.concatenate([_arr(seq, np.uint8), np.zeros(32, np.uint8)])
        rg_tid, rg_st, rg_en = _arr(rg_tid, np.int32), _arr(rg_st, np.uint64), _arr(rg_en, np.uint64)
        n, nr = len(tid), len(rg_tid)
        n_pos = int((rg_en.astype(np.int64) - rg_st.astype(np.int64)).sum()) if nr else 0

        class View(C.Structure):
            _fields_ = [("n_reads", C.c_uint64), ("ops", C.c_void_p), ("op_off", C.c_void_p), ("seq", C.c_void_p), ("seq_off", C.c_void_p),
                        ("l_seq", C.c_void_p), ("tid", C.c_void_p), ("pos", C.c_void_p), ("flag", C.c_void_p)]
        v = View(n, ops.ctypes.data, op_off.ctypes.data, seq.ctypes.data, seq_off.ctypes.data, l_seq.ctypes.data, tid.ctypes.data,
                 pos.ctypes.data, flag.ctypes.data)
        counts = np.zeros((max(n_pos, 1), 4), np.uint32)
        status = np.zeros(max(n, 1), np.uint32)
        ctr = np.zeros(6, np.uint64)
        self._chk(self.L.rb_host_nucfreq(self.ctx, C.byref(v), C.c_uint64(nr), _p(rg_tid), _p(rg_st), _p(rg_en), _p(counts), _p(status),
                                         _p(ctr)), "rb_host_nucfreq")
        return counts[:n_pos], status[:n], dict(max_depth=int(ctr[0]), n_covered=int(ctr[1]), n_bad=int(ctr[2]), unsorted=int(ctr[3]),
                                                    n_dropped=int(ctr[4]), cap_overflow=int(ctr[5]))

    # ---- nucfreq: the lines (k_nftext.hip) ----
    def nucfreq_text_scratch_bytes(self, n_seg, n_pos):
        f = self.L.rb_nucfreq_text_scratch_bytes
        f.restype = C.c_size_t
        return int(f(C.c_uint64(n_seg), C.c_uint64(n_pos)))

    def dev_nucfreq_text(self, counts, seg_cnt, seg_pos, seg_n, strings, pre_off, pre_len, suf_off, suf_len, mode, seg_text_off, seg_first,
                         seg_lines, text, text_cap, scratch, check=True):
        """counts, strings, the three segment outputs, text and scratch are device addresses (int); the seven segment arrays are host
        arrays (or None).  Enqueues on the context's stream.  Returns the call's return value (check=False: without raising)."""
        n_seg = len(seg_n) if seg_n is not None else 0
        h = [None if a is None else _arr(a, dt) for a, dt in ((seg_cnt, np.uint64), (seg_pos, np.uint64), (seg_n, np.uint32), (pre_off, np.uint32),
                                                              (pre_len, np.uint32), (suf_off, np.uint32), (suf_len, np.uint32))]
        q = [None if a is None else _p(a) for a in h]
        rc = self.L.rb_dev_nucfreq_text(self.ctx, C.c_void_p(counts), C.c_uint64(n_seg), q[0], q[1], q[2], C.c_void_p(strings), q[3], q[4], q[5], q[6],
                                        C.c_int(mode), C.c_void_p(seg_text_off), C.c_void_p(seg_first), C.c_void_p(seg_lines), C.c_void_p(text),
                                        C.c_uint64(text_cap), C.c_void_p(scratch))
        if check:
            self._chk(rc, "rb_dev_nucfreq_text")
        return int(rc)

    def nucfreq_text(self, tid, pos, flag, op_off, ops, l_seq, seq_off, seq, rg_tid, rg_st, rg_en, seg_cnt, seg_pos, seg_n, strings=b"",
                     pre_off=None, pre_len=None, suf_off=None, suf_len=None, mode=NFT_FULL):
        """Reads x regions as nucfreq(), the lines of the segments instead of the counts (rb_host_nucfreq_text).  Returns (slabs,
        read_status, counters): slabs = [(first_seg, seg_text_off [n + 1], seg_first [n], text bytes)] in segment order."""
        tid, pos, flag = _arr(tid, np.int32), _arr(pos, np.int64), _arr(flag, np.uint32)
        op_off, ops = _arr(op_off, np.uint64), np.concatenate([_arr(ops, np.uint32), np.zeros(4, np.uint32)])
        l_seq, seq_off = _arr(l_seq, np.uint32), _arr(seq_off, np.uint64)
        seq = np.concatenate([_arr(seq, np.uint8), np.zeros(32, np.uint8)])
        rg_tid, rg_st, rg_en = _arr(rg_tid, np.int32), _arr(rg_st, np.uint64), _arr(rg_en, np.uint64)
        seg_cnt, seg_pos, seg_n = _arr(seg_cnt, np.uint64), _arr(seg_pos, np.uint64), _arr(seg_n, np.uint32)
        fix = [None if a is None else _arr(a, np.uint32) for a in (pre_off, pre_len, suf_off, suf_len)]
        sb = np.frombuffer(bytes(strings) + b"\0", np.uint8).copy()
        n, nr = len(tid), len(rg_tid)

        class View(C.Structure):
            _fields_ = [("n_reads", C.c_uint64), ("ops", C.c_void_p), ("op_off", C.c_void_p), ("seq", C.c_void_p), ("seq_off", C.c_void_p),
                        ("l_seq", C.c_void_p), ("tid", C.c_void_p), ("pos", C.c_void_p), ("flag", C.c_void_p)]
        v = View(n, ops.ctypes.data, op_off.ctypes.data, seq.ctypes.data, seq_off.ctypes.data, l_seq.ctypes.data, tid.ctypes.data,
                 pos.ctypes.data, flag.ctypes.data)
        status = np.zeros(max(n, 1), np.uint32)
        ctr = np.zeros(6, np.uint64)
        slabs = []
        SINK = C.CFUNCTYPE(None, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint8))

        def sink(_user, first_seg, k, off, first, text):
            o = np.ctypeslib.as_array(off, (k + 1,)).copy()
            slabs.append((int(first_seg), o, np.ctypeslib.as_array(first, (k,)).copy(), C.string_at(text, int(o[k])) if int(o[k]) else b""))
        cb = SINK(sink)
        self._chk(self.L.rb_host_nucfreq_text(self.ctx, C.byref(v), C.c_uint64(nr), _p(rg_tid), _p(rg_st), _p(rg_en), C.c_uint64(len(seg_n)),
                                              _p(seg_cnt), _p(seg_pos), _p(seg_n), _p(sb), C.c_uint64(len(strings)),
                                              *[None if a is None else _p(a) for a in fix], C.c_int(mode), _p(status), _p(ctr), cb, None),
                  "rb_host_nucfreq_text")
        return slabs, status[:n], dict(max_depth=int(ctr[0]), n_covered=int(ctr[1]), n_bad=int(ctr[2]), unsorted=int(ctr[3]),
                                       n_dropped=int(ctr[4]), cap_overflow=int(ctr[5]))

    # ---- nucfreq on resident reads (rb_devreads_nucfreq, rb_devreads_nucfreq_text) ----
    def devreads_nucfreq(self, n_reads, ops, op_off, seq, seq_off, l_seq, tid, pos, flag, rg_tid, rg_st, rg_en):
        """nucfreq() on reads that are resident: the eight read pointers are device addresses (int; ops and seq the bases of absolute
        op_off / seq_off, the others may point into their columns).  Returns what nucfreq() returns."""
        rg_tid, rg_st, rg_en = _arr(rg_tid, np.int32), _arr(rg_st, np.uint64), _arr(rg_en, np.uint64)
        nr = len(rg_tid)
        n_pos = int((rg_en.astype(np.int64) - rg_st.astype(np.int64)).sum()) if nr else 0
        v = ReadsView(n_reads, ops, op_off, seq, seq_off, l_seq, tid, pos, flag)
        counts = np.zeros((max(n_pos, 1), 4), np.uint32)
        status = np.zeros(max(n_reads, 1), np.uint32)
        ctr = np.zeros(6, np.uint64)
        self._chk(self.L.rb_devreads_nucfreq(self.ctx, C.byref(v), C.c_uint64(nr), _p(rg_tid), _p(rg_st), _p(rg_en), _p(counts), _p(status),
                                             _p(ctr)), "rb_devreads_nucfreq")
        return counts[:n_pos], status[:n_reads], dict(max_depth=int(ctr[0]), n_covered=int(ctr[1]), n_bad=int(ctr[2]), unsorted=int(ctr[3]),
                                                      n_dropped=int(ctr[4]), cap_overflow=int(ctr[5]))

    def devreads_nucfreq_text(self, n_reads, ops, op_off, seq, seq_off, l_seq, tid, pos, flag, rg_tid, rg_st, rg_en, seg_cnt, seg_pos, seg_n,
                              strings=b"", pre_off=None, pre_len=None, suf_off=None, suf_len=None, mode=NFT_FULL):
        """nucfreq_text() on reads that are resident (device addresses as in devreads_nucfreq()).  Returns what nucfreq_text() returns."""
        rg_tid, rg_st, rg_en = _arr(rg_tid, np.int32), _arr(rg_st, np.uint64), _arr(rg_en, np.uint64)
        seg_cnt, seg_pos, seg_n = _arr(seg_cnt, np.uint64), _arr(seg_pos, np.uint64), _arr(seg_n, np.uint32)
        fix = [None if a is None else _arr(a, np.uint32) for a in (pre_off, pre_len, suf_off, suf_len)]
        sb = np.frombuffer(bytes(strings) + b"\0", np.uint8).copy()
        v = ReadsView(n_reads, ops, op_off, seq, seq_off, l_seq, tid, pos, flag)
        status = np.zeros(max(n_reads, 1), np.uint32)
        ctr = np.zeros(6, np.uint64)
        slabs = []
        SINK = C.CFUNCTYPE(None, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint8))

        def sink(_user, first_seg, k, off, first, text):
            o = np.ctypeslib.as_array(off, (k + 1,)).copy()
            slabs.append((int(first_seg), o, np.ctypeslib.as_array(first, (k,)).copy(), C.string_at(text, int(o[k])) if int(o[k]) else b""))
        cb = SINK(sink)
        self._chk(self.L.rb_devreads_nucfreq_text(self.ctx, C.byref(v), C.c_uint64(len(rg_tid)), _p(rg_tid), _p(rg_st), _p(rg_en), C.c_uint64(len(seg_n)),
                                                  _p(seg_cnt), _p(seg_pos), _p(seg_n), _p(sb), C.c_uint64(len(strings)),
                                                  *[None if a is None else _p(a) for a in fix], C.c_int(mode), _p(status), _p(ctr), cb, None),
                  "rb_devreads_nucfreq_text")
        return slabs, status[:n_reads], dict(max_depth=int(ctr[0]), n_covered=int(ctr[1]), n_bad=int(ctr[2]), unsorted=int(ctr[3]),
                                             n_dropped=int(ctr[4]), cap_overflow=int(ctr[5]))


def synth_n_ops(seed, first_record, n_rec, lo, hi):
    L = lib()
    return np.array([L.rb_synth_n_ops(seed, first_record + i, lo, hi) for i in range(n_rec)], dtype=np.uint64)


def synth_fill_ops_host(seed, first_record, op_off):
    L = lib()
    op_off = _arr(op_off, np.uint64)
    ops = np.zeros(int(op_off[-1]), np.uint32)
    L.rb_synth_fill_ops_host(C.c_uint64(seed), C.c_uint64(first_record), C.c_uint64(len(op_off) - 1), _p(op_off),
                             _p(ops))
    return ops


class DevBuf:
    """Device memory from the LIBRARY's allocator (rb_dev_alloc: what a host of the C ABI is told to use for a resident batch --
    requests of 256 MB and more are pieced together from 2 MB physical chunks, which decides 10-15 % of the streaming kernels' time,
    DESIGN.md section 3), seen by torch through the CUDA array interface without a copy: `.t` is the tensor.  free() gives the
    memory back (before the engine is closed)."""

    def __init__(self, eng, torch, n, dtype, device=None, placed_tries=1, score=None):
        self.eng, self.n, self.dtype = eng, int(n), dtype
        self.item = torch.empty(0, dtype=dtype).element_size()
        self.placement = None                       # (placed_tries > 1: {"sweep_ms": [...], "kept": i} of rb_dev_alloc_placed)

        def take():
            if placed_tries > 1:
                ptr, ms, kept = eng.dev_alloc_placed(max(self.n * self.item, 256), placed_tries, score)
                self.placement = {("launch_ms" if score else "sweep_ms"): ms, "kept": kept}
                return ptr
            return eng.dev_alloc(max(self.n * self.item, 256))
        try:
            self.ptr = take()
        except Exception:
            torch.cuda.empty_cache()                # (memory torch's caching allocator holds but does not use is not free to the driver)
            self.ptr = take()
        self.chunked = eng.L.rb_dev_alloc_mode(eng.ctx, C.c_void_p(self.ptr)) == 1  # (False: plain hipMalloc memory -- small, or the fallback)
        self.__cuda_array_interface__ = {"shape": (self.n * self.item,), "typestr": "|u1", "data": (self.ptr, False), "version": 3}
        try:
            self.t = torch.as_tensor(self, device=device if device is not None else "cuda").view(dtype)
            if device is not None and self.t.device != torch.device(device):
                raise RuntimeError(f"the buffer was taken for {self.t.device}, not {device}")
        except Exception:
            self.t = None
            eng.dev_free(self.ptr)
            self.ptr = 0
            raise

    def free(self):
        if self.ptr:
            self.t = None
            self.eng.dev_free(self.ptr)
            self.ptr = 0

    def release(self):
        """give the buffer back to the context (rb_dev_release): it stays mapped and keeps its pages for the next DevBuf of this size"""
        if self.ptr:
            self.t = None
            self.eng.dev_release(self.ptr)
            self.ptr = 0
